"""Host side of the K-models-in-one-launch route for the small policies (nic_small_rollout_ensemble_*): the slice sizes and the
validator of csrc/small_ensemble_plan.h through a stand-alone program built with the host compiler, the C declarations against
their ctypes prototypes, the [K][P] weight packing, the gradient views and the refusals that need no device."""
import copy
import os
import re
import shutil
import subprocess

import pytest
import torch

from golden_io import Golden
from neural_inventory_control_amd import _lib, build, ensemble_step as es, small_ensemble as se, small_rollout as sr
from neural_inventory_control_amd.neural_networks import NeuralNetworkCreator
from neural_inventory_control_amd.policy_layers import materialize_linears

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SLICES = ("weights", "rewards", "final_state", "states", "hidden", "logits", "slab_rows", "slab_row_stride", "slab", "grad", "scratch")
STRIDES = ("weights", "rewards", "final_state", "states", "hidden", "logits", "slab", "grad", "scratch")
# (B, ldb, T, F, n_hidden, n_out): cfg1 / cfg2 (one store), cfg4 (serial), a 3-slot store, one echelon, the widest chain
SHAPES = [(100, 128, 7, 4, 3, 1), (8192, 8192, 50, 4, 2, 1), (40, 64, 1, 15, 2, 4), (16, 64, 7, 3, 1, 1), (1000, 1024, 23, 11, 3, 3),
          (33, 64, 5, 16, 3, 8)]


def _host_clang():
    hipcc = os.path.realpath(shutil.which(build._hipcc()) or build._hipcc())
    for c in (os.path.join(os.path.dirname(hipcc), "..", "llvm", "bin", "clang++"), "/opt/rocm/llvm/bin/clang++",
              shutil.which("clang++"), shutil.which("g++")):
        if c and os.path.isfile(c):
            return c
    raise RuntimeError("no host C++ compiler to build tests/small_ensemble_plan_harness.cpp")


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("small_ensemble_plan") / "harness")
    # (-Wall -Werror: the header has to stay clean C++ for a compiler that knows nothing of HIP)
    subprocess.run([_host_clang(), "-O1", "-std=c++17", "-Wall", "-Werror", "-o", exe,
                    os.path.join(ROOT, "tests", "small_ensemble_plan_harness.cpp")], check=True)

    def run(*args):
        out = subprocess.run([exe] + [str(int(a)) if not isinstance(a, str) else a for a in args], check=True, capture_output=True,
                             text=True).stdout.strip()
        return out
    return run


def _slices(harness, shape, width):
    return dict(zip(SLICES, (int(v) for v in harness("slices", *shape, width).split())))


def test_build_hashes_the_plan_header():
    assert "small_ensemble_plan.h" in build.HEADERS
    assert "small_rollout_variants.h" in build.HEADERS and "small_rollout_mfma.h" in build.HEADERS


@pytest.mark.parametrize("shape", SHAPES)
def test_slice_sizes_are_what_the_single_model_engine_allocates(harness, shape):
    """FusedRollout._setup's sizes for the same shapes: histories [rows][T][ld] with NIC_SR16_STATE_ROWS / NIC_SR16_LOGIT_ROWS rows,
    slab [nic_small_rollout_bwd_wgrad_slots(B)][packed count rounded up to 4], the reduction's scratch."""
    B, ld, T, F, nh, no = shape
    lib = _lib.load_library()
    P0 = sr.packed_weight_count(F, nh, no)
    s16, s32 = _slices(harness, shape, 16), _slices(harness, shape, 32)
    for s in (s16, s32):
        assert s["weights"] == P0 and s["rewards"] == T * ld and s["final_state"] == F * ld
        assert s["hidden"] == nh * sr.H * T * ld
        assert s["slab_row_stride"] == s["grad"] == (P0 + 3) // 4 * 4 and s["slab"] == s["slab_rows"] * s["slab_row_stride"]
        assert s["scratch"] == lib.nic_small_rollout_reduce_scratch(s["slab_rows"], s["slab_row_stride"], T * ld)
        assert int(harness("scratch", s["slab_rows"], s["slab_row_stride"], T * ld)) == s["scratch"]
    assert s16["states"] == (F + 3) // 4 * 4 * T * ld and s16["logits"] == (no if no == 1 else (no + 3) // 4 * 4) * T * ld
    assert s32["states"] == F * T * ld and s32["logits"] == no * T * ld
    assert s16["slab_rows"] == lib.nic_small_rollout_bwd_wgrad_slots(B) == -(-B // 16) and s32["slab_rows"] == -(-B // 32)
    # the library hands Python the header's numbers
    d = _lib.NicSmallRolloutDesc()
    d.n_scenarios, d.ldb, d.T, d.F, d.n_hidden, d.n_out = shape
    for width, want in ((16, s16), (32, s32), (0, s32)):
        d.lane_scenarios = width
        assert sr.ensemble_slices(d) == want
    assert int(harness("scratch", 0, 0, T * ld)) == lib.nic_small_rollout_reduce_scratch(0, 0, T * ld) <= s32["scratch"]


def test_slices_query_refuses_bad_sizes():
    d = _lib.NicSmallRolloutDesc()
    d.n_scenarios, d.ldb, d.T, d.F, d.n_hidden, d.n_out, d.lane_scenarios = 100, 128, 7, 4, 4, 1, 16
    with pytest.raises(_lib.NicError, match="bad sizes"):
        sr.ensemble_slices(d)
    d.n_hidden, d.lane_scenarios = 3, 8
    with pytest.raises(_lib.NicError, match="lane_scenarios"):
        sr.ensemble_slices(d)


def test_validator_accepts_and_refuses(harness):
    shape, width = (100, 128, 7, 15, 2, 4), 16
    s = _slices(harness, shape, width)
    exact = {k: s[k] for k in STRIDES}

    def fwd(n_models=3, with_history=1, **kw):
        st = {**exact, **kw}
        return int(harness("fwd", *shape, width, n_models, *[st[k] for k in STRIDES], with_history).split()[0])

    def bwd(n_models=3, row=None, **kw):
        st = {**exact, **kw}
        return int(harness("bwd", *shape, width, n_models, *[st[k] for k in STRIDES], s["slab_row_stride"] if row is None else row).split()[0])

    def red(n_models=3, with_slab=1, n_rows=None, row=None, P=None, with_rewards=1, n_el=None, **kw):
        st = {**exact, **kw}
        return int(harness("reduce", n_models, *[st[k] for k in STRIDES], with_slab, s["slab_rows"] if n_rows is None else n_rows,
                           s["slab_row_stride"] if row is None else row, s["grad"] if P is None else P, with_rewards,
                           s["rewards"] if n_el is None else n_el).split()[0])
    OK, MODELS, WEIGHTS, REWARDS, FINAL, STATES, HIDDEN, LOGITS, SLAB_ROW, SLAB, GRAD, SCRATCH, ALIGN = range(13)
    # accepted: the exact slices, one model, the most models, longer strides
    assert fwd() == bwd() == red() == OK
    assert fwd(n_models=1) == bwd(n_models=1) == red(n_models=1) == OK
    assert fwd(n_models=65535) == bwd(n_models=65535) == red(n_models=65535) == OK
    assert fwd(**{k: exact[k] + 8 for k in STRIDES}) == bwd(**{k: exact[k] + 8 for k in STRIDES}) == OK
    assert red(**{k: exact[k] + 8 for k in STRIDES}) == OK
    assert fwd(weights=exact["weights"] + 1) == OK    # (the packed weights are read as scalars: any stride >= the count)
    # model counts
    for n in (0, -1, 65536):
        assert fwd(n_models=n) == bwd(n_models=n) == red(n_models=n) == MODELS
    # every stride one short of its slice
    assert fwd(weights=exact["weights"] - 1) == bwd(weights=exact["weights"] - 1) == WEIGHTS
    assert fwd(rewards=exact["rewards"] - 4) == red(rewards=exact["rewards"] - 4) == REWARDS
    assert fwd(final_state=exact["final_state"] - 1) == FINAL
    for k, code in (("states", STATES), ("hidden", HIDDEN), ("logits", LOGITS)):
        assert fwd(**{k: exact[k] - 4}) == bwd(**{k: exact[k] - 4}) == code
        assert fwd(with_history=0, **{k: 0}) == OK            # evaluation: the history strides are not looked at
        assert fwd(**{k: exact[k] + 2}) == bwd(**{k: exact[k] + 2}) == ALIGN
    assert fwd(rewards=exact["rewards"] + 2) == red(rewards=exact["rewards"] + 2) == ALIGN
    # slab rows and slab
    assert bwd(row=s["weights"] - 1) == SLAB_ROW and bwd(row=s["weights"], slab=s["slab_rows"] * s["weights"]) == OK
    assert bwd(slab=exact["slab"] - 1) == SLAB and bwd(row=s["slab_row_stride"] + 4) == SLAB
    assert red(row=s["grad"] - 1) == SLAB_ROW and red(slab=exact["slab"] - 1) == SLAB and red(grad=exact["grad"] - 1) == GRAD
    assert red(scratch=exact["scratch"] - 1) == SCRATCH
    # costs only: the slab's strides are not looked at, the scratch is the smaller one
    small = int(harness("scratch", 0, 0, s["rewards"]))
    assert red(with_slab=0, slab=0, grad=0, scratch=small) == OK and red(with_slab=0, scratch=small - 1) == SCRATCH
    assert harness("fwd", *shape, width, 0, *[exact[k] for k in STRIDES], 1) == "1 n_models must be 1..65535"


ENTRY_POINTS = {"nic_small_rollout_ensemble_fwd": 8, "nic_small_rollout_ensemble_bwd_wgrad": 9, "nic_small_rollout_ensemble_reduce": 12,
                "nic_small_rollout_ensemble_slices": 2}
C_TYPES = {"const NicSmallRolloutDesc*": "LP_NicSmallRolloutDesc", "const NicSmallEnsemble*": "LP_NicSmallEnsemble",
           "NicSmallEnsembleSlices*": "LP_NicSmallEnsembleSlices", "float*": "c_void_p", "const float*": "c_void_p", "void*": "c_void_p",
           "NicTable2": "NicTable2", "int64_t": "c_long", "int32_t": "c_int"}


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


def test_ctypes_structs_mirror_the_header():
    with open(os.path.join(ROOT, "include", "nic_rollout.h")) as f:
        header = f.read()
    for cls in (_lib.NicSmallEnsemble, _lib.NicSmallEnsembleSlices):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (cls.__name__, cls.__name__), header, flags=re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields = []
        for decl in body.split(";"):
            decl = decl.strip()
            if decl:
                ctype, names = decl.split(None, 1)
                fields += [(n.strip(), ctype) for n in names.split(",")]
        want = {"int32_t": _lib.C.c_int32, "int64_t": _lib.C.c_int64}
        assert [(n, want[t]) for n, t in fields] == list(cls._fields_)


# ---- engine-side host logic ---------------------------------------------------------------------------------------------------------
def _models(name, k, hidden=None, activation=None, materialize=True):
    g = Golden(name)
    c = g.fresh_config()

    class _Sc:
        problem_params = c["problem_params"]
        store_params = {"demand": {"mean": [5.0]}}
    nn_params = copy.deepcopy(c["nn_params"])
    if hidden is not None:
        nn_params["neurons_per_hidden_layer"]["master"] = hidden
    if activation is not None:
        nn_params["inner_layer_activations"]["master"] = activation
    out = []
    for i in range(k):
        torch.manual_seed(100 + i)
        m = NeuralNetworkCreator().create_neural_network(_Sc(), nn_params, device="cpu")
        if materialize:
            F = g.params["net.master.0.weight"].shape[1]
            materialize_linears(m.master_linears(), F)
        out.append(m)
    return out, g


@pytest.mark.parametrize("name", ["cfg1_one_store_lost_vanilla", "cfg4_serial_vanilla"])
def test_packing_is_the_stack_of_the_single_model_packing(name):
    models, _ = _models(name, 3)
    lins = [m.master_linears() for m in models]
    want = torch.stack([sr.pack_weights(ls) for ls in lins])
    assert torch.equal(se.pack_ensemble_weights(lins), want)
    out = torch.full_like(want, float("nan"))
    assert se.pack_ensemble_weights(lins, out) is out and torch.equal(out, want)
    with pytest.raises(ValueError):
        se.pack_ensemble_weights(lins, torch.zeros(3, want.shape[1] + 1))


@pytest.mark.parametrize("name", ["cfg1_one_store_lost_vanilla", "cfg4_serial_vanilla"])
def test_gradient_views_map_to_the_right_parameter_of_the_right_model(name):
    """a [K][P] buffer filled with the packed weights themselves: every view must then equal its own parameter"""
    models, _ = _models(name, 3)
    lins = [m.master_linears() for m in models]
    F, nh, no = lins[0][0].in_features, len(lins[0]) - 1, lins[0][-1].out_features
    P0 = sr.packed_weight_count(F, nh, no)
    grad = torch.full((3, (P0 + 3) // 4 * 4 + 8), float("nan"))
    grad[:, :P0] = se.pack_ensemble_weights(lins)
    views = es.grad_views(grad, [F] + [sr.H] * nh + [no])
    assert len(views) == 3
    for ls, (gw, gb) in zip(lins, views):
        assert len(gw) == len(gb) == len(ls)
        for lin, w, b in zip(ls, gw, gb):
            assert w.shape == lin.weight.shape and b.shape == lin.bias.shape
            assert torch.equal(w, lin.weight.detach()) and torch.equal(b, lin.bias.detach())
            assert w.data_ptr() >= grad.data_ptr() and w._base is not None   # views, not copies


@pytest.mark.parametrize("F", [1, 3, 7])
@pytest.mark.parametrize("nh", [1, 2, 3])
@pytest.mark.parametrize("no", [1, 2])
def test_the_two_descriptions_of_the_packed_row_agree(F, nh, no):
    """ensemble_step's layout on dims = [F, 32, ..., n_out] is small_rollout's on (F, n_hidden, n_out)"""
    dims = [F] + [32] * nh + [no]
    assert es.layer_slices(dims) == sr.layer_slices(F, nh, no)
    assert es.packed_count(dims) == sr.packed_weight_count(F, nh, no)


def test_model_lists_that_are_refused_without_a_device():
    good, _ = _models("cfg1_one_store_lost_vanilla", 2, materialize=False)
    assert se.check_models(good) == good
    with pytest.raises(ValueError, match="at least one"):
        se.SmallPolicyEnsemble([], {}, "cpu")
    narrow, _ = _models("cfg1_one_store_lost_vanilla", 1, hidden=[32, 32], materialize=False)
    with pytest.raises(ValueError, match="model 1: architecture"):
        se.SmallPolicyEnsemble(good[:1] + narrow, {}, "cpu")
    wide, _ = _models("cfg1_one_store_lost_vanilla", 1, hidden=[64, 64], materialize=False)
    with pytest.raises(ValueError, match="model 0: .*hidden layers of 32"):
        se.SmallPolicyEnsemble(wide, {}, "cpu")
    relu, _ = _models("cfg1_one_store_lost_vanilla", 1, activation="relu", materialize=False)   # not FusedRollout's either
    with pytest.raises(ValueError, match="model 1: SmallPolicyEnsemble handles the ELU MLP policies"):
        se.SmallPolicyEnsemble(good[:1] + relu, {}, "cpu")
    with pytest.raises(ValueError, match="model 0"):
        se.SmallPolicyEnsemble([torch.nn.Linear(4, 1)], {}, "cpu")
    serial, _ = _models("cfg4_serial_vanilla", 2, materialize=False)
    with pytest.raises(ValueError, match="model 1: architecture"):
        se.SmallPolicyEnsemble(good[:1] + serial[:1], {}, "cpu")
    serial[1].warehouse_upper_bound = torch.tensor([123.0])
    serial[0].warehouse_upper_bound = torch.tensor([124.0])
    with pytest.raises(ValueError, match="model 1: warehouse_upper_bound"):
        se.SmallPolicyEnsemble(serial, {}, "cpu")
