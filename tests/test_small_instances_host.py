"""Host side of K small policies on I problem instances (nic_small_rollout_instances_*): the validator, the model -> instance rule and
the offsets of csrc/small_ensemble_plan.h through a stand-alone program built with the host compiler, the C declarations against
their ctypes prototypes, and the engine's refusals that need no device."""
import os
import re
import subprocess

import pytest
import torch

from golden_io import Golden
from neural_inventory_control_amd import _lib, small_ensemble as se, small_rollout as sr
from neural_inventory_control_amd.layout import EnvProblem
from test_small_ensemble_host import _host_clang

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRIDES = ("demand", "state0", "underage", "holding", "lead", "wh_holding", "wh_lead", "wh_edge", "ech_holding", "ech_lead")
TABLES = STRIDES[2:]
OK, COUNT, DIVIDE, GRID, NEGATIVE, DEMAND, STATE0, ALIGN, NULL_TABLE = range(9)
REASONS = {COUNT: "n_instances must be at least 1", DIVIDE: "n_instances must divide n_models",
           GRID: "n_instances and the replicas per instance must be at most 65535", NEGATIVE: "negative instance stride",
           DEMAND: "demand stride shorter than (t0 + T) * ldb", STATE0: "state0 stride shorter than F * ldb",
           ALIGN: "the strides of demand and state0 must be multiples of 4 floats",
           NULL_TABLE: "instance stride for a table whose pointer is NULL"}


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("small_instances_plan") / "harness")
    # (-Wall -Werror: the header has to stay clean C++ for a compiler that knows nothing of HIP)
    subprocess.run([_host_clang(), "-O1", "-std=c++17", "-Wall", "-Werror", "-o", exe,
                    os.path.join(ROOT, "tests", "small_instances_plan_harness.cpp")], check=True)

    def run(*args):
        return subprocess.run([exe] + [a if isinstance(a, str) else str(int(a)) for a in args], check=True, capture_output=True,
                              text=True).stdout.strip()
    return run


def test_validator_accepts_the_natural_strides_and_names_every_refusal(harness):
    t0, T, ldb, F = 2, 7, 128, 15
    natural = dict(demand=(t0 + T) * ldb, state0=F * ldb, underage=ldb, holding=1, lead=ldb, wh_holding=1, wh_lead=1, wh_edge=0,
                   ech_holding=2, ech_lead=2 * ldb)

    def check(n_models=6, n_instances=3, present=None, full=False, **kw):
        st = {**natural, **kw}
        flags = [0 if present is not None and name not in present else 1 for name in TABLES]
        if present is None:
            flags[TABLES.index("wh_edge")] = 0   # (a setting without edge costs: the table is NULL and has no stride)
        out = harness("check", n_models, n_instances, *[st[k] for k in STRIDES], t0, T, ldb, F, *flags)
        return out if full else int(out.split()[0])

    # accepted: the natural strides, everything shared, one instance, as many instances as models, longer strides, the grid's limits
    assert check() == OK and check(full=True) == "0 accepted"
    assert check(**{k: 0 for k in STRIDES}) == OK
    assert check(n_instances=1) == check(n_instances=6) == check(n_instances=2) == OK
    assert check(demand=natural["demand"] + 8, state0=natural["state0"] + 4, underage=ldb + 3, holding=5) == OK
    assert check(n_models=65535, n_instances=65535) == check(n_models=65535, n_instances=1) == OK
    # the counts
    assert check(n_instances=0) == check(n_instances=-2) == COUNT
    assert check(n_instances=4) == check(n_models=6, n_instances=12) == DIVIDE
    assert check(n_models=2 * 65536, n_instances=65536) == check(n_models=2 * 65536, n_instances=2) == GRID
    # the strides
    for k in STRIDES:
        assert check(**{k: -4}) == NEGATIVE, k
    assert check(demand=natural["demand"] - 4) == DEMAND and check(demand=4) == DEMAND
    assert check(state0=natural["state0"] - 4) == STATE0
    assert check(demand=natural["demand"] + 2) == check(state0=natural["state0"] + 1) == ALIGN
    assert check(wh_edge=1) == NULL_TABLE
    for k in TABLES:   # a stride for a table the descriptor does not have
        assert check(present=[t for t in TABLES if t != k], wh_edge=1 if k == "wh_edge" else 0) == (NULL_TABLE if natural[k] or k == "wh_edge" else OK)
    assert check(present=["underage", "holding", "lead"], wh_holding=0, wh_lead=0, ech_holding=0, ech_lead=0) == OK   # (one store alone)
    for code, reason in REASONS.items():
        kw = {COUNT: dict(n_instances=0), DIVIDE: dict(n_instances=4), GRID: dict(n_models=2 * 65536, n_instances=2),
              NEGATIVE: dict(lead=-1), DEMAND: dict(demand=8), STATE0: dict(state0=8), ALIGN: dict(state0=natural["state0"] + 2),
              NULL_TABLE: dict(wh_edge=3)}[code]
        assert check(full=True, **kw) == f"{code} {reason}"


@pytest.mark.parametrize("K,I", [(1, 1), (6, 1), (6, 2), (6, 3), (6, 6)])
def test_model_to_instance_map(harness, K, I):
    assert [int(v) for v in harness("map", K, I).split()] == [m // (K // I) for m in range(K)]


def test_the_kernels_multiply_and_shift_is_the_division(harness):
    assert harness("magic") == "ok"
    assert [int(v) for v in harness("map", 65535, 5).split()] == [m // 13107 for m in range(65535)]
    assert [int(v) for v in harness("map", 65535, 65535).split()] == list(range(65535))


@pytest.mark.parametrize("instance", [0, 1, 5, 65534])
def test_offsets_are_instance_times_stride(harness, instance):
    strides = [7 * 128, 15 * 128, 128, 1, 3, 0, 9, 2, 256, 0]
    assert [int(v) for v in harness("offsets", instance, *strides).split()] == [instance * s for s in strides]
    big = [2 ** 33, 2 ** 32 + 4] + [0] * 8    # (offsets are 64-bit: past 2^31 floats)
    if instance:
        assert [int(v) for v in harness("offsets", instance, *big).split()][:2] == [instance * big[0], instance * big[1]]


def test_recorded_names_carry_the_instances_after_the_models(harness):
    assert harness("name", 0, 16, 3, 1, 8, 4) == "small_rollout16_fwd_kernel<3,one_store,models=8,instances=4>"
    assert harness("name", 1, 32, 2, 2, 6, 1) == "small_rollout_bwd_mfma_kernel<2,wgrad,serial,models=6,instances=1>"
    assert harness("name", 1, 32, 2, 0, 6, 0) == "small_rollout_bwd_mfma_kernel<2,wgrad,any,models=6>"   # (every other entry point: as it was)
    assert harness("name", 0, 16, 3, 1, 0, 0) == "small_rollout16_fwd_kernel<3,one_store>"


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------
ENTRY_POINTS = {"nic_small_rollout_instances_fwd": 9, "nic_small_rollout_instances_bwd_wgrad": 10}
C_TYPES = {"const NicSmallRolloutDesc*": "LP_NicSmallRolloutDesc", "const NicSmallEnsemble*": "LP_NicSmallEnsemble",
           "const NicSmallInstances*": "LP_NicSmallInstances", "float*": "c_void_p", "const float*": "c_void_p", "void*": "c_void_p",
           "NicTable2": "NicTable2", "int64_t": "c_long"}


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


def test_ctypes_struct_mirrors_the_header():
    with open(os.path.join(ROOT, "include", "nic_rollout.h")) as f:
        header = f.read()
    body = re.search(r"typedef struct NicSmallInstances \{(.*?)\} NicSmallInstances;", header, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [(n.strip(), decl.split(None, 1)[0]) for decl in body.split(";") if decl.strip() for n in decl.split(None, 1)[1].split(",")]
    want = {"int32_t": _lib.C.c_int32, "int64_t": _lib.C.c_int64}
    assert [(n, want[t]) for n, t in fields] == list(_lib.NicSmallInstances._fields_)
    assert tuple(n for n, _ in fields[2:]) == STRIDES == sr.INSTANCE_FIELDS
    assert _lib.C.sizeof(_lib.NicSmallInstances) == 8 + 8 * len(STRIDES)


def test_instance_strides_helper():
    inst = sr.instance_strides(3, demand=640, state0=256, underage=64)
    assert (inst.n_instances, inst.demand, inst.state0, inst.underage) == (3, 640, 256, 64)
    assert all(getattr(inst, k) == 0 for k in STRIDES[3:])
    with pytest.raises(KeyError):
        sr.instance_strides(2, weights=5)


def test_refused_without_a_device():
    """the entry points check before they touch the device: a request the validator refuses fails the same way on any machine"""
    lib = _lib.load_library()
    d = _lib.NicSmallRolloutDesc()
    d.n_scenarios, d.ldb, d.T, d.F, d.n_hidden, d.n_out, d.Ws = 40, 64, 3, 4, 2, 1, 4
    keep = torch.zeros(4096)
    d.weights = d.demand = d.state0 = keep.data_ptr()
    for name in ("underage", "holding", "lead"):
        setattr(d, name, _lib.NicTable2(keep.data_ptr(), 1, 0))
    sl = sr.ensemble_slices(d)
    ens = sr.ensemble_strides(4, **{k: sl[k] for k in ("weights", "rewards", "final_state")})
    out = torch.full((4, sl["rewards"]), float("nan"))
    for inst, reason in ((sr.instance_strides(3), REASONS[DIVIDE]), (sr.instance_strides(0), REASONS[COUNT]),
                         (sr.instance_strides(2, demand=64), REASONS[DEMAND]), (sr.instance_strides(2, wh_lead=1), REASONS[NULL_TABLE])):
        assert lib.nic_small_rollout_instances_fwd(d, ens, inst, out.data_ptr(), out.data_ptr(), None, None, None, None) != 0
        message = lib.nic_last_error().decode()
        assert message.startswith("nic_small_rollout_instances_fwd:") and reason in message, message
    assert bool(torch.isnan(out).all())


# ---- engine-side host logic -------------------------------------------------------------------------------------------------------------
def _problem(name="cfg1_one_store_lost_vanilla", B=None, underage=None, per_scenario=False):
    g = Golden(name)
    c = g.fresh_config()
    data = {k: (v[:B] if B else v).clone() for k, v in g.data.items()}
    if underage is not None:
        data["underage_costs"] = torch.full_like(data["underage_costs"], underage)
    if per_scenario:
        data["underage_costs"] = data["underage_costs"] + torch.arange(data["underage_costs"].shape[0], dtype=torch.float32)[:, None]
    return c["problem_params"], data, EnvProblem(c["problem_params"], data, "cpu")


def test_check_instances_accepts_a_cost_grid_and_names_the_first_mismatch():
    params, data, p0 = _problem(underage=4.0)
    grid = [p0] + [_problem(underage=u)[2] for u in (9.0, 19.0, 39.0)]
    assert se.check_instances(grid, 8) == 2 and se.check_instances(grid, 4) == 1 and se.check_instances([p0], 5) == 5
    lengths = [int(data["demands"].shape[2])] * 4
    assert se.check_instances(grid, 4, lengths) == 1
    with pytest.raises(ValueError, match="4 problem instances do not divide 6 models"):
        se.check_instances(grid, 6)
    with pytest.raises(ValueError, match="at least one problem instance"):
        se.check_instances([], 6)
    with pytest.raises(ValueError, match=r"instance 1: \d+ scenarios, instance 0 has \d+"):
        se.check_instances([p0, _problem(B=p0.B - 3)[2]], 2)
    with pytest.raises(ValueError, match="instance 2: a demand trace of 9 periods"):
        se.check_instances(grid, 4, [lengths[0], lengths[0], 9, lengths[0]])
    with pytest.raises(ValueError, match="instance 1: table 'underage' is per-scenario, instance 0's is uniform"):
        se.check_instances([p0, _problem(per_scenario=True)[2]], 2)
    flipped = _problem()[2]
    flipped.lost_demand = not p0.lost_demand
    with pytest.raises(ValueError, match="instance 1: lost_demand / maximize_profit"):
        se.check_instances([p0, flipped], 2)
    longer = _problem()[2]
    longer.Ws += 1
    with pytest.raises(ValueError, match="instance 1: pipeline shape"):
        se.check_instances([p0, longer], 2)


def test_stacked_tables_keep_instance_zero_first_and_give_the_strides():
    grid = [_problem(underage=u)[2] for u in (4.0, 9.0)] + [_problem(underage=19.0)[2]]
    stacked, strides = se.stack_instance_tables(grid)
    assert set(strides) == {"underage", "holding", "lead"}   # (one store: no warehouse or echelon tables, no strides for them)
    for name, stride in strides.items():
        t = getattr(stacked, name)
        assert t.tensor.shape[0] == 3 and stride == getattr(grid[0], name).tensor.numel() == t.tensor.stride(0)
        assert (t.loc_stride, t.scn_stride) == (getattr(grid[0], name).loc_stride, getattr(grid[0], name).scn_stride)
        for i, p in enumerate(grid):
            assert torch.equal(t.tensor[i], getattr(p, name).tensor)
    assert [float(stacked.underage.tensor[i].reshape(-1)[0]) for i in range(3)] == [4.0, 9.0, 19.0]
    assert getattr(grid[0], "underage").tensor.shape == stacked.underage.tensor.shape[1:]   # (the instances' own problems are untouched)
