"""K data_driven policies on I problem instances in one whole-horizon launch pair (`nic_horizon_rollout_instances_fwd / _bwd`,
`HorizonPolicyEnsemble` with a list of batches) against single-model launches / `FusedRollout.run` steps on each model's weights and
its instance's inputs, bit for bit.

The single-model kernels are refereed against a float64 rollout by tests/test_gpu_horizon.py; model m of an instances launch runs
their instruction stream on its own slices and on instance m // R's demand trace, initial state and tables, so the bar is
`torch.equal` - no tolerance - on every output, with NaN in every stride gap (models and instances alike), in every spare row and
padding column, and right behind every instance's demand slice of (t0 + T) periods.  Only the K totals are summed in another (fixed)
order than the single-model route's `torch.sum`: they are held to the project's 1e-5 relative bar."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import horizon_cases as hc  # noqa: E402
import test_gpu_horizon as single  # noqa: E402  (prepare / forward / backward of the single-model kernels: the yardstick)
import test_gpu_horizon_ensemble as ens  # noqa: E402  (_Launch: K models' weights and buffers with NaN gaps; _reference; _models)
import test_gpu_rollout as tgr  # noqa: E402  (the golden bars of the data_driven fixtures)
from golden_io import Golden  # noqa: E402
from neural_inventory_control_amd import _lib  # noqa: E402
from neural_inventory_control_amd import horizon_rollout as hz  # noqa: E402
from neural_inventory_control_amd.ensemble_adam import EnsembleAdam  # noqa: E402
from neural_inventory_control_amd.horizon_ensemble import HorizonPolicyEnsemble  # noqa: E402
from neural_inventory_control_amd.rollout import FusedRollout  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = single.DEV
_NAN = float("nan")
KERNEL_CASES = ens.KERNEL_CASES   # the seven cases that cover all six instantiations (B <= 40, T <= 5)
HISTORIES, DZ = ens.HISTORIES, ens.DZ
TABLES = ("underage", "holding", "lead", "wh_holding", "wh_lead", "wh_edge")   # EnvProblem's names = NicHorizonInstances' fields
IO_FIELD = dict(underage="underage", holding="holding", lead="lead_times", wh_holding="wh_holding", wh_lead="wh_lead_times",
                wh_edge="wh_edge_costs")
COST_SCALE = (1.0, 2.0, 0.5)


def _bits_equal(a, b):
    return ens._bits_equal(a, b)


def _perturb(L, i, traces=True, tables=True):
    """instance i of a prepared case, in place on the device (the descriptor's pointers stay): demand and initial pipelines times a
    seeded factor in [0.5, 1.5), underage costs times COST_SCALE[i] and the other costs times 1 + i / 2, store and warehouse lead
    times i periods shorter (at least 1; 0 stays 0: a pair without an edge in the shared mask).  Instance 0 is the case's own."""
    if i == 0:
        return L
    c = L.case
    prob, dem = L.keep
    gen = torch.Generator().manual_seed(100 + i)
    rand = lambda t: (0.5 + torch.rand(t.shape, generator=gen)).to(DEV)  # noqa: E731
    if traces:
        dem[:, :, :c.B] *= rand(dem[:, :, :c.B])
        L.state0[:, :c.B] *= rand(L.state0[:, :c.B])
    if tables:
        for name in TABLES:
            t = getattr(prob, name).tensor
            if t is None:
                continue
            if name in ("lead", "wh_lead"):
                t.copy_(torch.where(t > 0, (t - i).clamp_min(1.0), t))
            else:
                t.mul_(COST_SCALE[i] if name == "underage" else 1.0 + 0.5 * i)
    return L


def _single_run(c, m, i, traces=True, tables=True):
    """one single-model launch pair on instance i's inputs with model m's weights: every output as CPU tensors"""
    L = _perturb(single.prepare(c), i, traces, tables)
    w = ens._model_weights(c, m)
    for lin, (wn, bn) in zip(L.lin, (("W1", None), ("W2", "b2"), ("W3", "b3"))):
        lin.weight.copy_(w[wn].to(DEV))
        if bn:
            lin.bias.copy_(w[bn].to(DEV))
    L.z1_obs.live()[:] = w["z1_obs"].to(DEV)
    assert single.forward(L, with_hist=True) == hc.expected_kernels(c)[0]
    got = dict(rewards=L.rewards.live().cpu(), state_final=L.state_final.live().cpu(), **{n: h.live().cpu() for n, h in L.hist.items()})
    assert single.backward(L) == hc.expected_kernels(c)[1]
    got.update({n: h.live().cpu() for n, h in L.dz.items()})
    return got


_SINGLE = {}


def _reference(c, m, i, traces=True, tables=True):
    """computed once per (case, model, instance, what the instance changes), shared by the tests, never modified; instance 0 is the
    ensemble tests' own reference"""
    if i == 0 or not (traces or tables):
        return ens._reference(c, m)
    key = (c.id, m, i, traces, tables)
    if key not in _SINGLE:
        _SINGLE[key] = _single_run(c, m, i, traces, tables)
    return _SINGLE[key]


class _Stack:
    """I instances' copies of one input, instance i's i x stride floats behind instance 0's, stride = slice + gap, NaN in the gaps"""

    def __init__(self, parts, gap):
        self.n = parts[0].numel()
        self.stride = self.n + gap
        self.buf = torch.full((len(parts) * self.stride,), _NAN, device=DEV)
        for i, p in enumerate(parts):
            self.buf[i * self.stride:i * self.stride + self.n] = p.reshape(-1)
        self.before = self.buf.clone()

    def unchanged(self):
        return _bits_equal(self.buf, self.before)


class _Launch(ens._Launch):
    """descriptor, strides and buffers of a K-model launch of case `c` on I instances (traces / tables: what is per instance; the
    rest is shared, stride 0, instance 0's)"""

    def __init__(self, c, K, I, traces=True, tables=True):
        super().__init__(c, K)
        self.I, self.R = I, K // I
        Ls = [_perturb(single.prepare(c), i, traces, tables) for i in range(I)]
        self.keep_instances = Ls
        d, strides = self.desc, {}
        n_dem = (c.t0 + c.T) * c.S * c.ldb   # an instance's slice: NaN follows where a single-model trace has period t0 + T
        self.state0 = self.L.state0
        self.stacks = {}
        if traces:
            self.stacks["demand"] = _Stack([L.keep[1][:c.t0 + c.T] for L in Ls], 8)
            self.stacks["state0"] = _Stack([L.state0 for L in Ls], 4)
            assert self.stacks["demand"].n == n_dem
            d.demand = self.stacks["demand"].buf.data_ptr()
            self.state0 = self.stacks["state0"].buf
            strides.update(demand=self.stacks["demand"].stride, state0=self.stacks["state0"].stride)
        if tables:
            for k, name in enumerate(TABLES):
                t0 = getattr(Ls[0].keep[0], name)
                if t0.tensor is None:
                    continue
                assert t0.tensor.is_contiguous()
                st = self.stacks[name] = _Stack([getattr(L.keep[0], name).tensor for L in Ls], 3 + k)   # (read as scalars: any gap)
                getattr(d.io, IO_FIELD[name]).p = st.buf.data_ptr()
                strides[name] = st.stride
        self.inst = hz.instance_strides(I, **strides)
        self.inst_strides = strides

    def forward(self, with_hist=True, with_final=True):
        h = [self.hist[n].buf for n in HISTORIES] if with_hist else [None] * 5
        hz.horizon_instances_fwd(self.desc, self.ens, self.inst, self.z1_obs.buf, self.state0, self.rewards.buf,
                                 self.state_final.buf if with_final else None, *h)
        torch.cuda.synchronize()
        return _lib.lib().nic_last_kernel().decode()

    def backward(self):
        hz.horizon_instances_bwd(self.desc, self.ens, self.inst, *(self.hist[n].buf for n in HISTORIES), self.L.g_reward,
                                 *(self.dz[n].buf for n in DZ))
        torch.cuda.synchronize()
        return _lib.lib().nic_last_kernel().decode()


def _names(c, K, I):
    return tuple(n[:-1] + f",models={K},instances={I}>" for n in hc.expected_kernels(c))


def _check_launch(E, traces=True, tables=True):
    c, K = E.c, E.K
    for m in range(K):
        ref = _reference(c, m, m // E.R, traces, tables)
        for n, b in E.outputs.items():
            got = b.live(m).cpu()
            got = got[0] if n == "rewards" else got
            want = ref[n][0] if n == "rewards" else ref[n]
            assert not bool(torch.isnan(got).any()), (c.id, m, n, "a NaN from a gap or from behind a demand slice")
            assert torch.equal(got.reshape(want.shape), want), (c.id, m, n)
    for n, b in E.outputs.items():
        assert b.outside_untouched(), (c.id, n, "written outside a model's (row < rows, t < T, b < B)")
    assert E.inputs_unchanged() and all(s.unchanged() for s in E.stacks.values())


SHAPES = [(c, 4, 2) for c in KERNEL_CASES] + [(single._case("ref"), 3, 3)]


@pytest.mark.parametrize("c,K,I", SHAPES, ids=[f"{c.id}-K{K}-I{I}" for c, K, I in SHAPES])
def test_instances_launch_is_single_model_launches_on_each_instance(c, K, I):
    E = _Launch(c, K, I)
    assert E.inst.n_instances == I and all(v > 0 for v in E.inst_strides.values())
    assert {"demand", "state0", "underage", "holding", "lead"} <= set(E.inst_strides)
    want_fwd, want_bwd = _names(c, K, I)
    assert E.forward() == want_fwd
    assert E.backward() == want_bwd
    _check_launch(E)
    # the instances do differ, and so do the replicas of one instance: equal outputs are not one run copied K times
    R = K // I
    assert not torch.equal(_reference(c, 0, 0)["rewards"], _reference(c, R, 1)["rewards"])
    assert not torch.equal(_reference(c, R, 1)["rewards"], ens._reference(c, R)["rewards"])
    if R > 1 and c.id == "ref":
        assert not torch.equal(_reference(c, R, 1)["dz1_hist"], _reference(c, R + 1, 1)["dz1_hist"])


@pytest.mark.parametrize("traces,tables", [(False, True), (True, False)], ids=["tables-only", "traces-only"])
def test_demand_and_state_shared_with_tables_per_instance_and_the_reverse(traces, tables):
    c = single._case("ref")
    E = _Launch(c, 4, 2, traces, tables)
    shared = ("demand", "state0") if not traces else TABLES
    assert all(getattr(E.inst, k) == 0 for k in shared) and any(getattr(E.inst, k) > 0 for k in hz.INSTANCE_FIELDS)
    assert E.forward() == _names(c, 4, 2)[0] and E.backward() == _names(c, 4, 2)[1]
    _check_launch(E, traces, tables)
    assert not torch.equal(_reference(c, 2, 1, traces, tables)["rewards"], ens._reference(c, 2)["rewards"])


@pytest.mark.parametrize("id", ["ref", "FD161", "min"])
def test_one_instance_with_zero_strides_is_the_ensemble_launch(id):
    c = single._case(id)
    A, B_ = _Launch(c, 3, 1, traces=False, tables=False), ens._Launch(c, 3)
    assert all(getattr(A.inst, k) == 0 for k in hz.INSTANCE_FIELDS) and not A.stacks
    assert A.forward() == _names(c, 3, 1)[0] and A.backward() == _names(c, 3, 1)[1]
    # the ensemble entry points keep their names
    assert B_.forward() == ens._ensemble_names(c, 3)[0] and B_.backward() == ens._ensemble_names(c, 3)[1]
    for n in A.outputs:
        assert _bits_equal(A.outputs[n].buf, B_.outputs[n].buf), (id, n)
    _check_launch(A, False, False)


def test_forward_without_histories_and_refusals_launch_nothing():
    lib, p = _lib.lib(), _lib.ptr
    c = single._case("ref")
    E = _Launch(c, 4, 2)
    assert E.forward(with_hist=False) == _names(c, 4, 2)[0]
    for m in range(4):
        ref = _reference(c, m, m // 2)
        assert torch.equal(E.rewards.live(m).cpu(), ref["rewards"]) and torch.equal(E.state_final.live(m).cpu(), ref["state_final"])
    assert E.rewards.outside_untouched() and E.state_final.outside_untouched() and all(h.all_untouched() for h in E.hist.values())
    E.rewards.buf.fill_(_NAN)
    E.state_final.buf.fill_(_NAN)

    def refused(inst, word):
        st = lib.nic_horizon_rollout_instances_fwd(E.desc, E.ens, inst, p(E.z1_obs.buf), p(E.state0), p(E.rewards.buf), p(E.state_final.buf),
                                                   *(p(E.hist[n].buf) for n in HISTORIES), None)
        sb = lib.nic_horizon_rollout_instances_bwd(E.desc, E.ens, inst, *(p(E.hist[n].buf) for n in HISTORIES), E.L.g_reward.t2(),
                                                   *(p(E.dz[n].buf) for n in DZ), None)
        torch.cuda.synchronize()
        msg = lib.nic_last_error().decode()
        assert st != 0 and sb != 0 and word in msg, (word, msg)
        assert all(b.all_untouched() for b in E.outputs.values()), word

    s = E.inst_strides
    refused(hz.instance_strides(3, **s), "n_instances must divide n_models")
    refused(hz.instance_strides(0, **s), "n_instances must be 1..65535")
    refused(hz.instance_strides(2, **{**s, "demand": E.stacks["demand"].n - 4}), "demand stride shorter")
    refused(hz.instance_strides(2, **{**s, "state0": E.stacks["state0"].n - 4}), "state0 stride shorter")
    refused(hz.instance_strides(2, **{**s, "state0": s["state0"] + 2}), "multiples of 4 floats")
    refused(hz.instance_strides(2, **{**s, "lead": 8}), "lead-time stride shorter")
    refused(hz.instance_strides(2, **{**s, "wh_lead": -s["wh_lead"]}), "negative instance stride")
    # after all that the same buffers still take a good request
    assert E.forward() == _names(c, 4, 2)[0]
    assert torch.equal(E.rewards.live(3).cpu(), _reference(c, 3, 1)["rewards"])


# ---- engine ---------------------------------------------------------------------------------------------------------------------
NAME = ens.ENGINE_CASES[0]   # the real-data many-warehouse fixture
K_ENGINE = 4


def _instance_batch(data, i):
    """instance i of the fixture batch (0: the batch itself), perturbed as the launch-level instances are; the tables keep their
    layout (uniform stays uniform)"""
    if i == 0:
        return data
    gen = torch.Generator().manual_seed(100 + i)
    rand = lambda t: (0.5 + torch.rand(t.shape, generator=gen)).to(t.device)  # noqa: E731
    out = dict(data)
    for k in ("demands", "initial_inventories", "initial_warehouse_inventories"):
        out[k] = (data[k] * rand(data[k])).contiguous()
    for k in ("underage_costs", "holding_costs", "warehouse_holding_costs", "warehouse_edge_costs"):
        if data.get(k) is not None:
            out[k] = (data[k] * (COST_SCALE[i] if k == "underage_costs" else 1.0 + 0.5 * i)).contiguous()
    for k in ("lead_times", "warehouse_lead_times"):
        v = data[k].float()
        out[k] = torch.where(v > 0, (v - i).clamp_min(1.0), v).to(data[k].dtype).contiguous()
    return out


class _Setting:
    def __init__(self):
        self.g = Golden(NAME)
        self.c = self.g.fresh_config()
        self.data = {k: v.to(DEV) for k, v in self.g.data.items()}
        self.batches = [_instance_batch(self.data, i) for i in range(2)]
        self.T, self.ignore, self.obs, self.params = self.c["periods"], self.c["ignore"], self.c["observation_params"], self.c["problem_params"]
        self._want = None

    def models(self, k=K_ENGINE):
        return ens._models(self.g, self.g.fresh_config(), k=k)

    def engine(self, k=K_ENGINE, models=None, bound=False, model_gemms=True):
        e = HorizonPolicyEnsemble(models or self.models(k), self.params, DEV)
        e.model_gemms = model_gemms
        if bound:
            e.bind_parameters()
        return e

    def want(self):
        """per model m of K_ENGINE: its own FusedRollout step on instance m // 2's batch (computed once, never modified)"""
        if self._want is None:
            models = self.models()
            self._want = [ens._single_steps([m], self.c, self.batches[i // 2])[0] for i, m in enumerate(models)]
        return self._want


_S = []


def _setting():
    if not _S:
        _S.append(_Setting())
    return _S[0]


def test_engine_on_a_list_matches_single_model_steps_on_each_instance():
    s = _setting()
    want = s.want()
    models = s.models()
    e = s.engine(models=models)
    ev = e.run(s.batches, s.T, s.ignore, train=False, observation_params=s.obs)
    torch.cuda.synchronize()
    assert e.hist is None and e.grad is None
    ens._check(e, models, ev, want, train=False)
    tt = e.run(s.batches, s.T, s.ignore, train=True, observation_params=s.obs)
    torch.cuda.synchronize()
    ens._check(e, models, tt, want)   # per-period rewards, final state and every gradient bit-equal; the totals to 1e-5
    assert torch.equal(tt[0], ev[0]) and torch.equal(tt[1], ev[1])
    assert e.last_kernels["fwd"].endswith(",models=4,instances=2>") and e.last_kernels["bwd"].endswith(",models=4,instances=2>")
    assert e.last_kernels["z1"].endswith(",models=4>")
    # the instances differ, and the replicas of one instance differ
    assert want[0][0] != want[2][0] and want[0][0] != want[1][0] and want[2][0] != want[3][0]
    # model 0 is the fixture's policy on the unmodified fixture batch: the golden vectors, at the bars of test_gpu_rollout.py
    g, c = s.g, s.c
    torch.testing.assert_close(e.per_period_rewards()[0].cpu(), g.tensor("rewards").float(), rtol=1e-5, atol=2e-2)
    assert abs(float(tt[0][0]) - float(g.z["total"])) <= 1e-5 * abs(float(g.z["total"]))
    assert abs(float(tt[1][0]) - float(g.z["reported"])) <= 1e-5 * abs(float(g.z["reported"]))
    final = e.final_state(0)
    for k, v in g.states(c["periods"]).items():
        torch.testing.assert_close(final[k].cpu(), v.float(), rtol=2e-6, atol=2e-3)
    tgr._check_grads(models[0], g, tgr.GRAD_TOL)
    # the per-model GEMM loop gives the same bits
    loop = s.engine(model_gemms=False)
    tl = loop.run(s.batches, s.T, s.ignore, train=True, observation_params=s.obs)
    torch.cuda.synchronize()
    assert _bits_equal(tl[0], tt[0]) and _bits_equal(tl[1], tt[1])
    for name in ("rewards", "final", "z1", "grad"):
        assert _bits_equal(getattr(loop, name), getattr(e, name)), name
    assert not loop.last_kernels["z1"].endswith(",models=4>")


def test_two_train_steps_on_a_list_equal_two_engines_one_per_instance():
    s = _setting()
    lrs = (1e-3, 3e-3, 1e-2, 2e-3)
    models = s.models()
    e = s.engine(models=models, bound=True)
    P = e.weights.shape[1]
    opt = EnsembleAdam(4, P, DEV, lr=list(lrs), param_shapes=e.param_shapes)
    twins = s.models()
    halves = []
    for i in range(2):
        h = s.engine(models=twins[2 * i:2 * i + 2], bound=True)
        halves.append((h, EnsembleAdam(2, P, DEV, lr=list(lrs[2 * i:2 * i + 2]), param_shapes=h.param_shapes)))
    start = e.weights.clone()
    assert _bits_equal(start, torch.cat([h.weights for h, _ in halves]))
    for _ in range(2):
        got = e.train_step(s.batches, s.T, s.ignore, opt, s.obs)
        want = [h.train_step(s.batches[i], s.T, s.ignore, o, s.obs) for i, (h, o) in enumerate(halves)]
        torch.cuda.synchronize()
        for j in (0, 1):
            a, b = got[j], torch.cat([w[j] for w in want])
            assert _bits_equal(a, b)   # (the same fixed-order reduction per model on both sides)
    assert _bits_equal(e.weights, torch.cat([h.weights for h, _ in halves]))
    assert _bits_equal(e.grad, torch.cat([h.grad for h, _ in halves]))
    assert _bits_equal(opt.exp_avg, torch.cat([o.exp_avg for _, o in halves])) and opt.steps().tolist() == [2] * 4
    assert bool(torch.isfinite(e.weights).all()) and all(not torch.equal(e.weights[m], start[m]) for m in range(4))
    assert halves[0][0].last_kernels["fwd"].endswith(",models=2>")   # a dict batch: the ensemble entry points, as before


def test_a_dict_after_a_list_and_the_reverse_give_what_they_give_alone():
    s = _setting()
    run = lambda e, d, **kw: e.run(d, s.T, s.ignore, observation_params=s.obs, **kw)  # noqa: E731
    alone_list, alone_dict = s.engine(), s.engine()
    tl = run(alone_list, s.batches)
    td = run(alone_dict, s.batches[1])
    torch.cuda.synchronize()
    keep = lambda e: [getattr(e, n).clone() for n in ("rewards", "final", "grad")]  # noqa: E731
    want_list, want_dict = keep(alone_list), keep(alone_dict)
    for order in ((s.batches, s.batches[1], s.batches), (s.batches[1], s.batches, s.batches[1])):
        e = s.engine()
        for d in order:
            tt = run(e, d)
            torch.cuda.synchronize()
            listed = isinstance(d, list)
            wt, wb = (tl, want_list) if listed else (td, want_dict)
            assert _bits_equal(tt[0], wt[0]) and _bits_equal(tt[1], wt[1]), listed
            assert all(_bits_equal(a, b) for a, b in zip(keep(e), wb)), listed
            assert e.last_kernels["fwd"].endswith(",models=4,instances=2>" if listed else ",models=4>")
    # other batches of the same shape: the stacked tables are refreshed
    fresh = s.engine()
    ts, tf = run(alone_list, s.batches[::-1]), run(fresh, s.batches[::-1])
    torch.cuda.synchronize()
    assert _bits_equal(ts[0], tf[0]) and all(_bits_equal(a, b) for a, b in zip(keep(alone_list), keep(fresh)))
    assert not torch.equal(alone_list.rewards, want_list[0])
    # mismatches between the instances are named before anything is launched
    with pytest.raises(ValueError, match="3 problem instances do not divide 4 models"):
        run(e, [s.data] * 3)
    short = {k: v[:5].contiguous() for k, v in s.data.items()}
    with pytest.raises(ValueError, match=r"instance 1: \d+ scenarios, instance 0 has \d+"):
        run(e, [s.data, short])


def test_fit_on_list_batches_tracks_the_best_dev_loss_per_model():
    s = _setting()
    e = s.engine(bound=True)
    opt = EnsembleAdam(4, e.weights.shape[1], DEV, lr=[1e-3, 3e-3, 1e-2, 2e-3], param_shapes=e.param_shapes)
    B = s.data["demands"].shape[0]
    halves = [[{k: v[lo:hi].contiguous() for k, v in b.items()} for b in s.batches] for lo, hi in ((0, B // 2), (B // 2, B))]
    train_hist, dev_hist = e.fit(halves, [s.batches], 2, s.T, s.T, s.ignore, opt, s.obs)
    torch.cuda.synchronize()
    assert train_hist.shape == dev_hist.shape == (2, 4) and bool(torch.isfinite(train_hist).all()) and bool(torch.isfinite(dev_hist).all())
    assert e.best_dev.shape == (4,) and torch.equal(e.best_dev.cpu(), dev_hist.cpu().min(dim=0).values)
    assert e.best_weights.shape == e.weights.shape and opt.steps().tolist() == [4] * 4
    # the dev loss of epoch 0 is an evaluation of the list after two steps: per (scenario, reported period, store), per instance
    assert float(dev_hist[0, 0]) != float(dev_hist[0, 2])
