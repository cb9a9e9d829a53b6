"""Host side of K data_driven policies on I problem instances (nic_horizon_rollout_instances_*): the validator, the model -> instance
rule, the slices and the offsets of csrc/horizon_ensemble_plan.h through a stand-alone program built with the host compiler, the C
declarations against their ctypes prototypes, the entry points' refusals (made before anything touches the device) and the
engine's refusals that need no device."""
import os
import re
import subprocess

import pytest
import torch

from golden_io import Golden
from neural_inventory_control_amd import _lib, ensemble_step, horizon_ensemble as he, horizon_rollout as hz, small_ensemble as se
from neural_inventory_control_amd.layout import EnvProblem
from test_horizon_ensemble_host import _host_clang

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRIDES = ("demand", "state0", "underage", "holding", "lead", "wh_holding", "wh_lead", "wh_edge")
TABLES = STRIDES[2:]
(OK, COUNT, DIVIDE, GRID, NEGATIVE, DEMAND, STATE0, ALIGN, NULL_TABLE, UNDERAGE, HOLDING, LEAD, WH_HOLDING, WH_LEAD, WH_EDGE) = range(15)
REASONS = {COUNT: "n_instances must be 1..65535", DIVIDE: "n_instances must divide n_models",
           GRID: "the replicas per instance must be at most 65535", NEGATIVE: "negative instance stride",
           DEMAND: "demand stride shorter than (t0 + T) * S * ldb", STATE0: "state0 stride shorter than the state rows x ldb",
           ALIGN: "the strides of demand and state0 must be multiples of 4 floats",
           NULL_TABLE: "instance stride for a table whose pointer is NULL", UNDERAGE: "underage stride shorter than the table",
           HOLDING: "holding stride shorter than the table", LEAD: "lead-time stride shorter than the table",
           WH_HOLDING: "warehouse-holding stride shorter than the table", WH_LEAD: "warehouse-lead-time stride shorter than the table",
           WH_EDGE: "warehouse-edge-cost stride shorter than the table"}
# the real-data batch's shape with a period shift: 21 stores x 3 warehouses, pipelines of 6 / 3 slots, 72 products in 128 columns
S, WN, WS, WW, B, LDB, T, T0 = 21, 3, 6, 3, 72, 128, 9, 2
SHAPE = (S, WN, WS, WW, B, LDB, T, T0)
# per table: present, loc_stride, [sup_stride,] scn_stride - underage per scenario ([S][ldb]), holding uniform ([S]), lead times per
# scenario ([S][Wn][ldb]), warehouse holding uniform, warehouse lead times per scenario, no edge costs
LAYOUT = dict(underage=(1, LDB, 1), holding=(1, 1, 0), lead=(1, WN * LDB, LDB, 1), wh_holding=(1, 1, 0), wh_lead=(1, LDB, 1),
              wh_edge=(0, 0, 0))
EXTENT = dict(underage=(S - 1) * LDB + B, holding=S, lead=(S - 1) * WN * LDB + (WN - 1) * LDB + B, wh_holding=WN,
              wh_lead=(WN - 1) * LDB + B, wh_edge=1)   # (wh_edge: the NULL table's all-zero strides span one float)
NATURAL = dict(demand=(T0 + T) * S * LDB, state0=(S * WS + WN * WW) * LDB, underage=S * LDB, holding=S, lead=S * WN * LDB,
               wh_holding=WN, wh_lead=WN * LDB, wh_edge=0)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("horizon_instances_plan") / "harness")
    # (-Wall -Werror: the header has to stay clean C++ for a compiler that knows nothing of HIP)
    subprocess.run([_host_clang(), "-O1", "-std=c++17", "-Wall", "-Werror", "-o", exe,
                    os.path.join(ROOT, "tests", "horizon_instances_plan_harness.cpp")], check=True)

    def run(*args):
        return subprocess.run([exe] + [a if isinstance(a, str) else str(int(a)) for a in args], check=True, capture_output=True,
                              text=True).stdout.strip()
    return run


def _tables(layout):
    return [v for name in TABLES for v in layout[name]]


def _check(harness, n_models=6, n_instances=3, layout=None, full=False, **kw):
    st = {**NATURAL, **kw}
    out = harness("check", n_models, n_instances, *[st[k] for k in STRIDES], *SHAPE, *_tables(layout or LAYOUT))
    return out if full else int(out.split()[0])


def test_slices_are_what_the_kernels_address(harness):
    """demand: periods t0 .. t0 + T - 1 of [S][ldb] rows (neither kernel reads period t0 + T); state0 [F_dyn][ldb]; a table: from its
    first element to one past element (last row, last supplier, scenario B - 1)"""
    got = [int(v) for v in harness("slices", *SHAPE, *_tables(LAYOUT)).split()]
    assert got[:2] == [NATURAL["demand"], NATURAL["state0"]]
    assert dict(zip(TABLES, got[2:])) == EXTENT
    assert all(EXTENT[k] <= NATURAL[k] for k in TABLES if LAYOUT[k][0])   # (the engine's stacked tables: one instance's tensor apart)


def test_validator_accepts_the_natural_strides_and_names_every_refusal(harness):
    check = lambda **kw: _check(harness, **kw)   # noqa: E731
    # accepted: the natural strides, everything shared, one instance, as many instances as models, longer strides, the grid's limits
    assert check() == OK and check(full=True) == "0 accepted"
    assert check(**{k: 0 for k in STRIDES}) == OK
    assert check(n_instances=1) == check(n_instances=6) == check(n_instances=2) == OK
    assert check(demand=NATURAL["demand"] + 8, state0=NATURAL["state0"] + 4, underage=NATURAL["underage"] + 3, holding=S + 5) == OK
    assert check(demand=0) == check(state0=0) == check(lead=0) == OK            # (traces shared, tables per instance; the reverse)
    assert check(**{k: 0 for k in TABLES}) == OK
    # the counts: 65535 and 65536, instances and replicas
    assert check(n_models=65535, n_instances=65535) == check(n_models=65535, n_instances=1) == OK
    assert check(n_models=65536, n_instances=65536) == COUNT and check(n_models=65536, n_instances=1) == GRID
    assert check(n_models=2 * 65536, n_instances=2) == GRID and check(n_models=2 * 65535, n_instances=2) == OK
    assert check(n_instances=0) == check(n_instances=-2) == COUNT
    # I dividing K, then not
    assert check(n_models=6, n_instances=3) == OK and check(n_models=6, n_instances=4) == DIVIDE and check(n_models=6, n_instances=12) == DIVIDE
    # no negative stride
    for k in STRIDES:
        assert check(**{k: -4}) == NEGATIVE, k
    # every stride equal to its slice, then one float short (the aligned ones: also the next multiple of 4 below)
    exact = dict(demand=NATURAL["demand"], state0=NATURAL["state0"], **{k: EXTENT[k] for k in TABLES if LAYOUT[k][0]})
    assert check(**exact) == OK
    for k, code in (("demand", DEMAND), ("state0", STATE0), ("underage", UNDERAGE), ("holding", HOLDING), ("lead", LEAD),
                    ("wh_holding", WH_HOLDING), ("wh_lead", WH_LEAD)):
        assert check(**{k: exact[k]}) == OK, k
        assert check(**{k: exact[k] - 1}) == code, k
    assert check(demand=exact["demand"] - 4) == DEMAND and check(state0=exact["state0"] - 4) == STATE0 and check(demand=4) == DEMAND
    # the demand and state0 strides are multiples of 4 floats (tables are read as scalars: any stride)
    assert check(demand=exact["demand"] + 2) == check(state0=exact["state0"] + 1) == ALIGN
    assert check(underage=exact["underage"] + 1, lead=exact["lead"] + 3) == OK
    # a stride on a NULL table: the setting's missing edge costs, then every table in turn
    assert check(wh_edge=0) == OK and check(wh_edge=1) == NULL_TABLE
    edge = {**LAYOUT, "wh_edge": (1, 1, 0)}
    assert _check(harness, layout=edge, wh_edge=WN) == OK and _check(harness, layout=edge, wh_edge=WN - 1) == WH_EDGE
    for k in TABLES[:-1]:
        gone = {**LAYOUT, k: (0,) + LAYOUT[k][1:]}
        assert _check(harness, layout=gone) == NULL_TABLE and _check(harness, layout=gone, **{k: 0}) == OK, k
    # a stores-only setting: no warehouse tables, no strides for them
    assert harness("check", 4, 2, 8 * 5 * 64, 3 * 5 * 64, 5, 5, 5, 0, 0, 0, 5, 0, 3, 0, 40, 64, 8, 0,
                   1, 1, 0, 1, 1, 0, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0) == "0 accepted"
    for code, reason in REASONS.items():
        kw = {COUNT: dict(n_instances=0), DIVIDE: dict(n_instances=4), GRID: dict(n_models=2 * 65536, n_instances=2),
              NEGATIVE: dict(lead=-1), DEMAND: dict(demand=8), STATE0: dict(state0=8), ALIGN: dict(state0=NATURAL["state0"] + 2),
              NULL_TABLE: dict(wh_edge=3), UNDERAGE: dict(underage=8), HOLDING: dict(holding=2), LEAD: dict(lead=8),
              WH_HOLDING: dict(wh_holding=1), WH_LEAD: dict(wh_lead=8)}.get(code)
        if code == WH_EDGE:
            assert _check(harness, layout=edge, wh_edge=1, full=True) == f"{code} {reason}"
        else:
            assert check(full=True, **kw) == f"{code} {reason}"


@pytest.mark.parametrize("K,I", [(1, 1), (4, 2), (6, 3), (6, 1), (5, 5)])
def test_model_to_instance_map(harness, K, I):
    """model m runs on instance m // R, R = K / I: the rule of csrc/small_ensemble_plan.h (the harness also holds the kernels'
    multiply and shift to it)"""
    assert [int(v) for v in harness("map", K, I).split()] == [m // (K // I) for m in range(K)]


def test_the_kernels_multiply_and_shift_is_the_division(harness):
    assert harness("magic") == "ok"
    assert [int(v) for v in harness("map", 65535, 5).split()] == [m // 13107 for m in range(65535)]
    assert [int(v) for v in harness("map", 65535, 65535).split()] == list(range(65535))


def test_all_zero_strides_are_the_shared_request(harness):
    assert harness("shared", *[0] * 8) == "1"
    for k in range(8):
        assert harness("shared", *[4 if j == k else 0 for j in range(8)]) == "0"
    inst = hz.instance_strides(1)
    assert inst.n_instances == 1 and all(getattr(inst, k) == 0 for k in STRIDES)


@pytest.mark.parametrize("instance", [0, 1, 5, 65534])
def test_offsets_are_instance_times_stride_and_null_stays_null(harness, instance):
    strides = [11 * 21 * 128, 135 * 128, 21 * 128, 21, 63, 0, 3 * 128, 0]
    want = [str(instance * s) if s or j < 2 else "null" for j, s in enumerate(strides)]
    assert harness("offsets", instance, *strides).split() == want
    big = [2 ** 33, 2 ** 32 + 4] + [0] * 6    # (offsets are 64-bit: past 2^31 floats)
    if instance:
        assert [int(v) for v in harness("offsets", instance, *big).split()[:2]] == [instance * big[0], instance * big[1]]


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------
ENTRY_POINTS = {"nic_horizon_rollout_instances_fwd": 13, "nic_horizon_rollout_instances_bwd": 13}
C_TYPES = {"const NicHorizonDesc*": "LP_NicHorizonDesc", "const NicHorizonEnsemble*": "LP_NicHorizonEnsemble",
           "const NicHorizonInstances*": "LP_NicHorizonInstances", "float*": "c_void_p", "const float*": "c_void_p", "void*": "c_void_p",
           "NicTable2": "NicTable2"}


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
    # the ensemble calls' buffers, in their order, behind the descriptor, the ensemble and the instances
    ens = re.search(r"int %s\(([^)]*)\);" % name.replace("_instances", "_ensemble"), header)
    one = [" ".join(a.split()) for a in ens.group(1).split(",")]
    assert [" ".join(a.split()) for a in m.group(1).split(",")] == one[:2] + ["const NicHorizonInstances* inst"] + one[2:]
    comment = header[:header.index("int %s(" % name)].rsplit("/*", 1)[1]
    assert "trainer.py:181-216" in comment and "once per model and setting" in comment and "neural_networks.py:430-515" in comment
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        assert name in f.read()
    assert hasattr(_lib.load_library(), name)


def test_ctypes_struct_mirrors_the_header():
    with open(os.path.join(ROOT, "include", "nic_rollout.h")) as f:
        header = f.read()
    body = re.search(r"typedef struct NicHorizonInstances \{(.*?)\} NicHorizonInstances;", header, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [(n.strip(), decl.split(None, 1)[0]) for decl in body.split(";") if decl.strip() for n in decl.split(None, 1)[1].split(",")]
    want = {"int32_t": _lib.C.c_int32, "int64_t": _lib.C.c_int64}
    assert [(n, want[t]) for n, t in fields] == list(_lib.NicHorizonInstances._fields_)
    assert tuple(n for n, _ in fields[2:]) == STRIDES == hz.INSTANCE_FIELDS
    assert _lib.C.sizeof(_lib.NicHorizonInstances) == 8 + 8 * len(STRIDES)


def test_instance_strides_helper():
    inst = hz.instance_strides(3, demand=640, state0=256, underage=64)
    assert (inst.n_instances, inst.demand, inst.state0, inst.underage) == (3, 640, 256, 64)
    assert all(getattr(inst, k) == 0 for k in STRIDES[3:])
    with pytest.raises(KeyError):
        hz.instance_strides(2, ech_lead=5)   # (no extra echelons on this route)
    with pytest.raises(KeyError):
        hz.instance_strides(2, W1=5)


def _descriptor(keep):
    """a descriptor the whole-horizon launchers accept (stores only: 5 stores, pipelines of 3), every pointer into CPU memory -
    nothing is read through them without a launch"""
    d = _lib.NicHorizonDesc()
    D = d.io.dims
    D.n_scenarios, D.ldb, D.n_stores, D.n_warehouses, D.store_slots, D.warehouse_slots, D.lost_demand = 40, 64, 5, 0, 3, 0, 1
    d.T, d.t0, d.H1, d.H2, d.n_out, d.ldw1, d.ldw2, d.ldw3, d.hist_stride = 4, 1, 32, 32, 5, 15, 32, 32, 4 * 64
    for name in ("W1", "W2", "W3", "b2", "b3", "demand"):
        setattr(d, name, keep.data_ptr())
    d.io.underage = _lib.NicTable2(keep.data_ptr(), 64, 1)
    d.io.holding = _lib.NicTable2(keep.data_ptr(), 1, 0)
    d.io.lead_times = _lib.NicTable3(keep.data_ptr(), 1, 0, 0)
    return d


def test_refused_without_a_device():
    """the entry points check before they touch the device: a request the validator refuses fails the same way on any machine"""
    lib = _lib.load_library()
    keep = torch.zeros(1 << 16)
    d = _descriptor(keep)
    sl = hz.ensemble_slices(d)
    ens = hz.ensemble_strides(4, **sl)
    out = torch.full((4, max(sl.values())), float("nan"))
    p, g = out.data_ptr(), _lib.NicTable2(keep.data_ptr(), 0, 0)
    demand, state0, underage = (1 + 4) * 5 * 64, 15 * 64, 4 * 64 + 40
    cases = ((hz.instance_strides(3), REASONS[DIVIDE]), (hz.instance_strides(0), REASONS[COUNT]), (hz.instance_strides(65536), REASONS[COUNT]),
             (hz.instance_strides(2, demand=demand - 4), REASONS[DEMAND]), (hz.instance_strides(2, state0=state0 - 4), REASONS[STATE0]),
             (hz.instance_strides(2, demand=demand + 2), REASONS[ALIGN]), (hz.instance_strides(2, underage=underage - 1), REASONS[UNDERAGE]),
             (hz.instance_strides(2, holding=4), REASONS[HOLDING]), (hz.instance_strides(2, lead=-5), REASONS[NEGATIVE]),
             (hz.instance_strides(2, wh_lead=1), REASONS[NULL_TABLE]), (hz.instance_strides(4, wh_edge=8), REASONS[NULL_TABLE]))
    for inst, reason in cases:
        for name, call in (("nic_horizon_rollout_instances_fwd", lambda: lib.nic_horizon_rollout_instances_fwd(
                                d, ens, inst, keep.data_ptr(), keep.data_ptr(), p, p, p, p, p, p, p, None)),
                           ("nic_horizon_rollout_instances_bwd", lambda: lib.nic_horizon_rollout_instances_bwd(
                                d, ens, inst, p, p, p, p, p, g, p, p, p, None))):
            assert call() != 0, (name, reason)
            message = lib.nic_last_error().decode()
            assert message.startswith(name + ":") and reason in message, message
    assert lib.nic_horizon_rollout_instances_fwd(d, ens, None, keep.data_ptr(), keep.data_ptr(), p, p, p, p, p, p, p, None) != 0
    assert "null ensemble / instances" in lib.nic_last_error().decode()
    assert lib.nic_horizon_rollout_instances_bwd(d, None, hz.instance_strides(1), p, p, p, p, p, g, p, p, p, None) != 0
    assert "null ensemble / instances" in lib.nic_last_error().decode()
    # the ensemble's own refusals come first, as in nic_horizon_rollout_ensemble_*
    assert lib.nic_horizon_rollout_instances_fwd(d, hz.ensemble_strides(0, **sl), hz.instance_strides(1), keep.data_ptr(), keep.data_ptr(),
                                                 p, p, p, p, p, p, p, None) != 0
    assert "n_models must be 1..65535" in lib.nic_last_error().decode()
    assert bool(torch.isnan(out).all())


# ---- engine-side host logic -------------------------------------------------------------------------------------------------------------
NAME = "f4_real_many_warehouses_data_driven"


def _problem(B=None, underage=None, per_scenario=False, **replace):
    g = Golden(NAME)
    c = g.fresh_config()
    data = {k: (v[:B] if B else v).clone() for k, v in g.data.items()}
    if underage is not None:
        data["underage_costs"] = data["underage_costs"] * underage
    if per_scenario:
        data["holding_costs"] = data["holding_costs"] + torch.arange(data["holding_costs"].shape[0], dtype=torch.float32)[:, None]
    data.update(replace)
    return c, data, EnvProblem(c["problem_params"], data, "cpu")


def test_check_instances_accepts_a_cost_grid_and_names_the_first_mismatch():
    c, d0, p0 = _problem()
    obs = c["observation_params"]
    grid = [(d0, p0)] + [_problem(underage=u)[1:] for u in (0.5, 2.0, 4.0)]
    datas, probs = [d for d, _ in grid], [p for _, p in grid]
    assert he.check_instances(probs, 8, datas, obs) == 2 and he.check_instances(probs, 4, datas, [obs] * 4) == 1
    assert he.check_instances(probs[:1], 5, datas[:1], obs) == 5
    with pytest.raises(ValueError, match="HorizonPolicyEnsemble: 4 problem instances do not divide 6 models"):
        he.check_instances(probs, 6, datas, obs)
    with pytest.raises(ValueError, match="HorizonPolicyEnsemble needs at least one problem instance"):
        he.check_instances([], 6, [], obs)
    _, d1, p1 = _problem(B=p0.B - 3)
    with pytest.raises(ValueError, match=r"instance 1: \d+ scenarios, instance 0 has \d+"):
        he.check_instances([p0, p1], 2, [d0, d1], obs)
    _, d1, p1 = _problem(demands=d0["demands"][:, :, :-1].clone())
    with pytest.raises(ValueError, match=r"instance 1: a demand trace of \d+ periods, instance 0's has \d+"):
        he.check_instances([p0, p1], 2, [d0, d1], obs)
    _, d1, p1 = _problem(initial_inventories=d0["initial_inventories"][:, :, :-1].clone())
    with pytest.raises(ValueError, match="instance 1: pipeline shape"):
        he.check_instances([p0, p1], 2, [d0, d1], obs)
    _, d1, p1 = _problem()
    p1.lost_demand = not p0.lost_demand
    with pytest.raises(ValueError, match="instance 1: lost_demand / maximize_profit"):
        he.check_instances([p0, p1], 2, [d0, d1], obs)
    _, d1, p1 = _problem(per_scenario=True)
    kinds = {p0.holding.scn_stride == 0, p1.holding.scn_stride == 0}
    assert kinds == {True, False}
    with pytest.raises(ValueError, match="instance 1: table 'holding' is (per-scenario|uniform), instance 0's is (uniform|per-scenario)"):
        he.check_instances([p0, p1], 2, [d0, d1], obs)
    _, d1, p1 = _problem()
    p1.wh_edge = copy_of = p1.wh_holding if p0.wh_edge.tensor is None else type(p1.wh_edge).null()
    assert (copy_of.tensor is None) != (p0.wh_edge.tensor is None)
    with pytest.raises(ValueError, match="instance 1: table 'wh_edge' is (missing|present), instance 0's is not"):
        he.check_instances([p0, p1], 2, [d0, d1], obs)
    # the policy's input row count: another past-demand window, another number of time features
    wider = {**obs, "demand": {**obs["demand"], "past_periods": obs["demand"]["past_periods"] + 1}}
    with pytest.raises(ValueError, match=r"instance 1: the policy's input has \d+ rows \(past-demand window, time features\), instance 0's \d+"):
        he.check_instances([p0, p0], 2, [d0, d0], [obs, wider])
    _, d1, p1 = _problem(days_from_christmas=torch.cat([d0["days_from_christmas"]] * 2, dim=1))
    with pytest.raises(ValueError, match=r"instance 1: the policy's input has \d+ rows"):
        he.check_instances([p0, p1], 2, [d0, d1], obs)
    shifted = {**obs, "demand": {**obs["demand"], "period_shift": obs["demand"]["period_shift"] + 1}}
    with pytest.raises(ValueError, match=r"instance 1: period_shift \d+ differs from instance 0's \d+"):
        he.check_instances([p0, p0], 2, [d0, d0], [obs, shifted])
    with pytest.raises(ValueError, match="3 observation_params for 2 problem instances"):
        he.check_instances([p0, p0], 2, [d0, d0], [obs] * 3)
    assert he.input_rows(p0, d0, obs) == Golden(NAME).params["net.master.0.weight"].shape[1]


def test_helpers_moved_to_the_shared_module_keep_their_names_and_messages():
    assert se.check_instances is ensemble_step.check_instances and se.stack_instance_tables is ensemble_step.stack_instance_tables
    _, _, p0 = _problem()
    with pytest.raises(ValueError, match="SmallPolicyEnsemble needs at least one problem instance"):
        se.check_instances([], 2)
    with pytest.raises(ValueError, match="SmallPolicyEnsemble: 2 problem instances do not divide 3 models"):
        se.check_instances([p0, p0], 3)
    stacked, strides = he.stack_instance_tables([p0, _problem(underage=2.0)[2]])
    assert set(strides) <= set(TABLES) and {"underage", "holding", "lead", "wh_holding", "wh_lead"} <= set(strides)
    for name, stride in strides.items():
        t = getattr(stacked, name)
        assert t.tensor.shape[0] == 2 and stride == getattr(p0, name).tensor.numel() == t.tensor.stride(0)
        assert torch.equal(t.tensor[0], getattr(p0, name).tensor)
    assert torch.equal(stacked.underage.tensor[1], stacked.underage.tensor[0] * 2.0)
