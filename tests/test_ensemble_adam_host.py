"""Host side of the ensemble Adam (nic_ensemble_adam_*, EnsembleAdam): csrc/ensemble_adam_body.h through a stand-alone program built
with the host compiler - against a float64 Adam with torch's own float32 Adam as the yardstick, its running products against pow,
its request checks - the C declarations against their ctypes prototypes, the build id, and what of `EnsembleAdam` needs no device."""
import copy
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import ensemble_adam_checks as eac
from golden_io import Golden
from neural_inventory_control_amd import _lib, build
from neural_inventory_control_amd.ensemble_adam import EnsembleAdam
from neural_inventory_control_amd.neural_networks import NeuralNetworkCreator
from neural_inventory_control_amd.policy_layers import materialize_linears
from neural_inventory_control_amd.trainer import _portable_optimizer_state

ROOT = eac.ROOT


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    d = tmp_path_factory.mktemp("ensemble_adam")
    return eac.build_harness(d), d


def test_body_is_as_close_to_float64_adam_as_torch_is(harness):
    """K = 3, P = 2,305, 5 steps.  The bar measures itself: the body's max |error| against float64 Adam is at most 2 x that of
    torch.optim.Adam (default, CPU, float32) on the same inputs, per model - both are float32 chains of the same few roundings
    and the final rounding of p dominates.  Observed: body 8.67e-08 / 5.97e-08 / 5.61e-08, torch the same (ratios 1.00)."""
    exe, d = harness
    K, P = 3, 2305
    params, grads, hyper = eac.inputs(P)
    zeros = np.zeros((K, P), dtype=np.float32)
    out = eac.run_harness(exe, d, P, params, grads, hyper, zeros, zeros, eac.fresh_state(K))
    assert list(out["state"]["step"]) == [eac.STEPS] * K
    ref = eac.adam_f64(params, grads, hyper)
    assert np.abs(ref - params).max() > 1e-3   # (the steps moved the parameters)
    for m in range(K):
        theirs, _ = eac.torch_adam(params[m], grads[:, m], hyper[m])
        err_body = float(np.abs(out["params"][m].astype(np.float64) - ref[m]).max())
        err_torch = float(np.abs(theirs.astype(np.float64) - ref[m]).max())
        print(f"model {m}: body {err_body:.3e}, torch {err_torch:.3e}, ratio {err_body / err_torch:.2f}")
        assert err_torch > 0.0
        assert err_body <= 2.0 * err_torch, (m, err_body, err_torch)


@pytest.mark.parametrize("beta", [0.8, 0.9, 0.999, 0.9995])
def test_running_product_against_pow(harness, beta):
    """at most t roundings of 2^-53 each: 2.2e-13 relative at t = 2,000, held to 1e-12"""
    exe, d = harness
    path = os.path.join(str(d), f"products_{beta}.bin")
    subprocess.run([exe, "products", repr(beta), "2000", path], check=True)
    got = np.fromfile(path, dtype="<f8")
    assert got.shape == (2000,)
    want = np.array([beta ** t for t in range(1, 2001)])
    assert np.all(want > 0)
    assert float((np.abs(got - want) / want).max()) <= 1e-12


def test_prepare_advances_the_state_and_rounds_the_coefficients_once(harness):
    exe, d = harness
    params, grads, hyper = eac.inputs(7)
    zeros = np.zeros((3, 7), dtype=np.float32)
    out = eac.run_harness(exe, d, 7, params, grads[:2], hyper, zeros, zeros, eac.fresh_state(3))
    for m, (lr, b1, b2, eps, wd) in enumerate(eac.HYPER):
        st = out["state"][m]
        assert st["step"] == 2 and st["c1"] == b1 * b1 and st["c2"] == b2 * b2
        want = [lr / (1.0 - b1 * b1), 1.0 / np.sqrt(1.0 - b2 * b2), b1, 1.0 - b1, b2, 1.0 - b2, eps, wd]
        assert np.array_equal(out["coef"][m], np.array(want, dtype=np.float64).astype(np.float32))


def test_columns_past_P_are_neither_read_nor_written(harness):
    """every stride P + another pad, NaN in every gap: the gaps keep their bits, the live columns are those of the exact strides"""
    exe, d = harness
    K, P = 3, 257
    params, grads, hyper = eac.inputs(P)
    zeros = np.zeros((K, P), dtype=np.float32)
    exact = eac.run_harness(exe, d, P, params, grads, hyper, zeros, zeros, eac.fresh_state(K))
    wide = eac.run_harness(exe, d, P, eac.padded(params, P + 3), eac.padded(grads, P + 5), hyper, eac.padded(zeros, P + 1),
                           eac.padded(zeros, P + 2), eac.fresh_state(K))
    for name in ("params", "exp_avg", "exp_avg_sq"):
        assert np.array_equal(eac.bits(wide[name][:, :P]), eac.bits(exact[name]))
        assert np.isnan(wide[name][:, P:]).all() and np.isfinite(wide[name][:, :P]).all()
    assert wide["state"].tobytes() == exact["state"].tobytes() and np.array_equal(wide["coef"], exact["coef"])


def test_request_checks(harness):
    exe, _ = harness

    def prepare(n_models=3, hyper=1, state=1, coef=1):
        out = subprocess.run([exe, "check_prepare"] + [str(v) for v in (n_models, hyper, state, coef)], check=True, capture_output=True,
                             text=True).stdout.strip()
        code, reason = out.split(" ", 1)
        assert reason and (int(code) == 0) == (reason == "accepted")
        return int(code)

    def update(n_models=3, P=2305, ptrs=(1, 1, 1, 1, 1), strides=None):
        strides = strides if strides is not None else (P, P, P, P)
        out = subprocess.run([exe, "check_update"] + [str(v) for v in (n_models, P, *ptrs, *strides)], check=True, capture_output=True,
                             text=True).stdout.strip()
        code, reason = out.split(" ", 1)
        assert reason and (int(code) == 0) == (reason == "accepted")
        return int(code), reason
    OK, MODELS, COLUMNS, NULL, PARAMS, GRADS, EXP_AVG, EXP_AVG_SQ = range(8)
    assert prepare() == update()[0] == OK
    assert prepare(n_models=1) == update(n_models=1)[0] == OK and prepare(n_models=65535) == update(n_models=65535)[0] == OK
    assert update(P=1)[0] == OK and update(strides=(2305, 2308, 2306, 4000))[0] == OK
    for n in (0, -1, 65536):
        assert prepare(n_models=n) == update(n_models=n)[0] == MODELS
    assert update(n_models=0) == (MODELS, "n_models must be 1..65535")
    assert update(P=0, strides=(4, 4, 4, 4))[0] == update(P=-3, strides=(4, 4, 4, 4))[0] == COLUMNS
    for i in range(3):
        assert prepare(**{("hyper", "state", "coef")[i]: 0}) == NULL
    for i in range(5):
        assert update(ptrs=tuple(0 if j == i else 1 for j in range(5)))[0] == NULL
    for i, code in enumerate((PARAMS, GRADS, EXP_AVG, EXP_AVG_SQ)):   # each stride one short
        got, reason = update(strides=tuple(2304 if j == i else 2305 for j in range(4)))
        assert got == code and "stride shorter than P" in reason


# ---- declarations, prototypes, build id ---------------------------------------------------------------------------------------------
ENTRY_POINTS = {"nic_ensemble_adam_prepare": 5, "nic_ensemble_adam_update": 12}
C_TYPES = {"float*": "c_void_p", "const float*": "c_void_p", "const double*": "c_void_p", "NicEnsembleAdamState*": "c_void_p",
           "void*": "c_void_p", "int64_t": "c_long", "int32_t": "c_int"}


@pytest.mark.parametrize("name", sorted(ENTRY_POINTS))
def test_entry_points_are_declared_and_bound_argument_for_argument(name):
    with open(os.path.join(ROOT, "include", "nic_rollout.h")) as f:
        header = f.read()
    m = re.search(r"int %s\(([^)]*)\);" % name, header)
    assert m, f"{name} is not declared in include/nic_rollout.h"
    declared = [" ".join(a.split()).rsplit(" ", 1)[0] for a in m.group(1).split(",")]
    res, args = _lib.PROTOTYPES[name]
    assert res is _lib.C.c_int and len(args) == len(declared) == ENTRY_POINTS[name]
    assert [C_TYPES[d] for d in declared] == [a.__name__ for a in args], (declared, args)
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        assert name in f.read()
    assert hasattr(_lib.load_library(), name)


def test_state_struct_mirrors_the_header_and_the_tensor_layout():
    with open(os.path.join(ROOT, "include", "nic_rollout.h")) as f:
        body = re.search(r"typedef struct NicEnsembleAdamState \{(.*?)\} NicEnsembleAdamState;", f.read(), flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [(n.strip(), decl.split(None, 1)[0]) for decl in body.split(";") if decl.strip() for n in decl.split(None, 1)[1].split(",")]
    want = {"int32_t": _lib.C.c_int32, "double": _lib.C.c_double}
    assert [(n, want[t]) for n, t in fields] == list(_lib.NicEnsembleAdamState._fields_)
    # EnsembleAdam keeps the state as three doubles a model with the counter in the first one's low half
    assert _lib.C.sizeof(_lib.NicEnsembleAdamState) == 24 == eac.STATE_DTYPE.itemsize
    assert (_lib.NicEnsembleAdamState.step.offset, _lib.NicEnsembleAdamState.c1.offset, _lib.NicEnsembleAdamState.c2.offset) == (0, 8, 16)


def test_build_compiles_the_unit_and_hashes_the_body_header(tmp_path):
    assert ("ensemble_adam.hip", ["-ffp-contract=off"]) in build.SOURCES
    assert "ensemble_adam_body.h" in build.HEADERS
    # the same tree shape as the package: <tmp>/pkg/csrc + <tmp>/include
    csrc = tmp_path / "pkg" / "csrc"
    csrc.mkdir(parents=True)
    (tmp_path / "include").mkdir()
    for src, _ in build.SOURCES:
        shutil.copy(os.path.join(build.CSRC, src), csrc / os.path.basename(src))
    for h in build.HEADERS:
        shutil.copy(os.path.join(build.CSRC, h), os.path.normpath(os.path.join(str(csrc), h)))
    before = build.source_id(str(csrc))
    assert before == build.source_id()
    with open(csrc / "ensemble_adam_body.h", "a") as f:
        f.write("// edited\n")
    assert build.source_id(str(csrc)) != before


# ---- EnsembleAdam without a device ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(lr=-1e-3), dict(lr=[1e-3, -1.0, 1e-3]), dict(lr=1e-3, betas=(1.0, 0.999)), dict(lr=1e-3, betas=(0.9, -0.1)),
                                dict(lr=1e-3, betas=([0.9, 0.9, 1.5], 0.999)), dict(lr=1e-3, eps=-1e-8), dict(lr=1e-3, weight_decay=-0.1),
                                dict(lr=float("nan")), dict(lr=[1e-3, 1e-3])])
def test_bad_hyper_parameters_are_refused_without_a_device(kw):
    with pytest.raises(ValueError, match="EnsembleAdam"):
        EnsembleAdam(3, 10, "cuda:0", **kw)   # (refused before anything touches the device)


def test_bad_sizes_and_setters_are_refused():
    for K, P in ((0, 10), (65536, 10), (3, 0)):
        with pytest.raises(ValueError):
            EnsembleAdam(K, P, "cpu", lr=1e-3)
    with pytest.raises(ValueError, match="param_shapes"):
        EnsembleAdam(2, 10, "cpu", lr=1e-3, param_shapes=[(3, 3)])
    opt = EnsembleAdam(3, 10, "cpu", lr=[1e-2, 3e-3, 1e-3], betas=(0.9, [0.999, 0.99, 0.9995]), weight_decay=[0.0, 1e-2, 0.0])
    assert opt.hyper_of(1) == dict(lr=3e-3, beta1=0.9, beta2=0.99, eps=1e-8, weight_decay=1e-2)
    with pytest.raises(ValueError):
        opt.set_lr([1e-3, 1e-3, -1e-3])
    with pytest.raises(ValueError):
        opt.set_betas((0.9, 1.0))
    assert opt.hyper_of(2)["lr"] == 1e-3 and opt.hyper_of(0)["beta2"] == 0.999   # a refused change writes nothing
    opt.set_lr(5e-4)
    opt.set_weight_decay([0.0, 0.0, 0.5])
    assert [opt.hyper_of(m)["lr"] for m in range(3)] == [5e-4] * 3 and torch.equal(opt.hyper, opt._hyper_host)
    assert opt.hyper_of(2)["weight_decay"] == 0.5
    with pytest.raises(_lib.NicUnavailableError):
        opt.step(torch.zeros(3, 10), torch.zeros(3, 10))


def _cpu_models(k):
    g = Golden("cfg1_one_store_lost_vanilla")
    c = g.fresh_config()

    class _Sc:
        problem_params = c["problem_params"]
        store_params = {"demand": {"mean": [5.0]}}
    out = []
    for i in range(k):
        torch.manual_seed(100 + i)
        m = NeuralNetworkCreator().create_neural_network(_Sc(), copy.deepcopy(c["nn_params"]), device="cpu")
        materialize_linears(m.master_linears(), g.params["net.master.0.weight"].shape[1])
        out.append(m)
    return out


def test_state_dict_round_trip_through_a_default_torch_adam():
    """the dict structure: `state_dict(m)` loads into a default torch.optim.Adam over model m's parameters, which steps with it, and
    what that optimizer saves loads back"""
    models = _cpu_models(2)
    shapes = [p.shape for p in models[0].parameters()]
    P = sum(s.numel() for s in shapes)
    opt = EnsembleAdam(2, P, "cpu", lr=[1e-2, 3e-3], betas=([0.9, 0.8], [0.999, 0.99]), eps=[1e-8, 1e-6], weight_decay=[0.0, 1e-2], param_shapes=shapes)
    gen = torch.Generator().manual_seed(5)
    opt.exp_avg.copy_(torch.randn(2, P, generator=gen))
    opt.exp_avg_sq.copy_(torch.rand(2, P, generator=gen))
    opt.state.view(torch.int32)[:, 0] = torch.tensor([3, 7], dtype=torch.int32)
    opt.state[:, 1] = torch.tensor([0.9 ** 3, 0.8 ** 7], dtype=torch.float64)
    opt.state[:, 2] = torch.tensor([0.999 ** 3, 0.99 ** 7], dtype=torch.float64)
    assert opt.steps().tolist() == [3, 7]
    m = 1
    sd = opt.state_dict(m)
    assert sorted(sd) == ["param_groups", "state"] and sorted(sd["state"]) == list(range(len(shapes))) and len(sd["param_groups"]) == 1
    g = sd["param_groups"][0]
    assert (g["lr"], g["betas"], g["eps"], g["weight_decay"], g["amsgrad"]) == (3e-3, (0.8, 0.99), 1e-6, 1e-2, False)
    assert g["beta1_power"] == 0.8 ** 7 and g["beta2_power"] == 0.99 ** 7 and g["params"] == list(range(len(shapes)))
    off = 0
    for i, s in enumerate(shapes):
        e = sd["state"][i]
        assert e["step"].device.type == "cpu" and e["step"].dtype == torch.float32 and float(e["step"]) == 7.0
        assert e["exp_avg"].shape == s and torch.equal(e["exp_avg"].reshape(-1), opt.exp_avg[m, off:off + s.numel()])
        assert e["exp_avg_sq"].shape == s and torch.equal(e["exp_avg_sq"].reshape(-1), opt.exp_avg_sq[m, off:off + s.numel()])
        off += s.numel()
    theirs = torch.optim.Adam(copy.deepcopy(models[m]).parameters())   # default: lr 1e-3
    theirs.load_state_dict(sd)
    tg = theirs.param_groups[0]
    assert (tg["lr"], tuple(tg["betas"]), tg["eps"], tg["weight_decay"]) == (3e-3, (0.8, 0.99), 1e-6, 1e-2)
    assert tg["beta1_power"] == 0.8 ** 7   # (torch keeps group keys it does not know)
    for p in tg["params"]:
        p.grad = torch.ones_like(p)
    theirs.step()   # the loaded state is one torch can step with
    assert all(float(theirs.state[p]["step"]) == 8.0 for p in tg["params"])
    # ... and back: torch's own dict (no running products in it once they are dropped) into a fresh EnsembleAdam
    back = _portable_optimizer_state(theirs.state_dict())
    for k in ("beta1_power", "beta2_power"):
        back["param_groups"][0].pop(k)
    fresh = EnsembleAdam(2, P, "cpu", lr=1.0, param_shapes=shapes)
    fresh.load_state_dict(m, back)
    assert fresh.steps().tolist() == [0, 8] and fresh.hyper_of(m) == dict(lr=3e-3, beta1=0.8, beta2=0.99, eps=1e-6, weight_decay=1e-2)
    assert fresh.hyper_of(0)["lr"] == 1.0 and torch.equal(fresh.hyper, fresh._hyper_host)
    assert fresh.state[m, 1].item() == 0.8 ** 8 and fresh.state[m, 2].item() == 0.99 ** 8
    flat = lambda name: torch.cat([theirs.state[p][name].reshape(-1) for p in tg["params"]])  # noqa: E731
    assert torch.equal(fresh.exp_avg[m], flat("exp_avg")) and torch.equal(fresh.exp_avg_sq[m], flat("exp_avg_sq"))
    assert float(fresh.exp_avg[0].abs().sum()) == 0.0
    # its own dict: the running products come back as they were
    again = EnsembleAdam(2, P, "cpu", lr=1.0, param_shapes=shapes)
    sd = opt.state_dict(m)   # (a fresh one: torch stepped the first one's `step` tensors in place)
    again.load_state_dict(m, sd)
    assert torch.equal(again.state[m], opt.state[m]) and torch.equal(again.exp_avg[m], opt.exp_avg[m])
    with pytest.raises(ValueError, match="amsgrad"):
        again.load_state_dict(m, {"state": sd["state"], "param_groups": [dict(g, amsgrad=True)]})
