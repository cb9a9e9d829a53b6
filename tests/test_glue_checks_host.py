"""The glue-kernel checkers (tests/glue_checks.py and the head checks of tests/kernel_checks.py) checked on the CPU: the tables
name every instantiation and every planted situation, the grid family's conditions hold on the reference alone, a plain float32
restatement of every kernel passes every case (and the host build of the three NIC_HD heads does), and every class of kernel
error the restatement can restate (`defect=`) fails at least one case."""
import pytest
import torch

import glue_checks as gc
import kernel_checks as kc

ALL = [(name, c) for name, (cases, _) in gc.CHECKERS.items() for c in cases]


# ---- 1. the tables ---------------------------------------------------------------------------------------------------------------

def test_case_ids_are_unique_and_listed():
    for name, (cases, _) in gc.CHECKERS.items():
        ids = [c.id for c in cases]
        assert len(ids) == len(set(ids)) and ids, name


def test_the_tables_reach_every_launcher_cell():
    """both segment-sum kernels <1> and <4>, gnn_alloc_env_{fwd,bwd}_kernel<4|8|16>, and every other launcher of the glue kernels"""
    names = gc.expected_kernel_names()
    assert names == gc.ALL_LAUNCHER_CELLS, (sorted(gc.ALL_LAUNCHER_CELLS - names), sorted(names - gc.ALL_LAUNCHER_CELLS))


def test_the_tables_name_every_path():
    has = lambda cases, pred: any(pred(c) for c in cases)  # noqa: E731
    # segment sums: R beyond gridDim.z = 32, both ways into <1>, a strided source, accumulate and scale both ways, every batch edge
    for cases in (gc.SEG_CASES, gc.TERMS_CASES):
        assert {1, 32, 33, 70} <= {c.R for c in cases}
        assert {"vec", "ld", "offset-dst", "offset-src"} <= {c.path for c in cases}
        assert {True, False} <= {c.hist for c in cases} and {True, False} <= {c.accumulate for c in cases}
        assert has(cases, lambda c: c.family == "random" and c.scale == "sqrt5")
    assert {None, "dyadic"} <= {c.scale for c in gc.SEG_CASES}
    assert set(gc.B_VEC) <= {c.B for c in gc.SEG_CASES if c.path == "vec"}
    assert set(kc.B_LANES256) <= {c.B for c in gc.SEG_CASES if c.path != "vec"}
    assert {0, 1, 3, 4, 5, 8, 9, 17} == set(gc.SEG_LENS)
    pats = {c.pattern for c in gc.TERMS_CASES}
    assert {len(p) for p in pats} == set(range(1, gc.NIC_SEG_MAX_TERMS + 1))
    for pos in range(gc.NIC_SEG_MAX_TERMS):      # plain and segment terms in every position
        assert {p[pos] for p in pats if len(p) > pos} == {"S", "P"}
    assert {(c.pattern[0], c.accumulate) for c in gc.TERMS_CASES} >= {("S", False), ("S", True), ("P", False), ("P", True)}
    # allocation: every S, self loop and cap both ways, both families, n_edges % 8 in {0, 1}, every batch edge
    assert {(c.S, c.e_self, c.cap, c.family) for c in gc.ALLOC_CASES} == {(S, s, k, f) for S in (1, 7, 8, 9, 16, 17, 64, 70)
                                                                         for s in (False, True) for k in (False, True)
                                                                         for f in ("grid", "random")}
    assert {c.n_edges % 8 for c in gc.ALLOC_CASES} == {0, 1} and set(kc.B_LANES64) <= {c.B for c in gc.ALLOC_CASES}
    assert {len(c.counts) for c in gc.GROUPS_CASES} == {1, 3, 5} and {n for c in gc.GROUPS_CASES for n in c.counts} == {0, 1, 8, 9}
    assert {c.Ww for c in gc.GROUPS_CASES} == {1, 3} and {c.zero_count > 0 for c in gc.GROUPS_CASES} == {True, False}
    assert set(kc.B_LANES64) <= {c.B for c in gc.GROUPS_CASES}
    for c in gc.GROUPS_CASES:      # the edge -> order row map is a real permutation
        rows = gc.alloc_layout(c)[4].tolist()
        assert rows[:sum(c.counts) + len(c.counts)] != sorted(rows[:sum(c.counts) + len(c.counts)]) or len(c.counts) == 1
    # fused allocation + env step
    ae = gc.ALLOC_ENV_CASES
    assert 18 <= len(ae) <= 24
    assert {c.S for c in ae} == {1, 3, 4, 5, 16, 17, 33} and {c.B for c in ae} == set(kc.B_LANES64)
    assert {(c.Ws, c.Ww) for c in ae} == {(2, 2), (4, 4), (5, 3), (3, 8), (9, 2), (16, 16)}
    for field in ("lost", "profit", "per_scenario", "e_self", "cap"):
        assert {getattr(c, field) for c in ae} == {True, False}, field
    # heads
    dd = kc.DATA_DRIVEN_CASES
    assert {7, 8, 9, 15, 16, 17, 23, 24, 25, 64, 70} <= {c.S for c in dd}
    assert {c.Wn for c in dd} == {0, 1, 2, 5} and {c.Ww for c in dd if c.Wn} == {1, 4, 16} and set(kc.B_LANES64) <= {c.B for c in dd}
    assert {c.E for c in kc.SERIAL_CASES} == {0, 1, 3} and {(c.Ww, c.We) for c in kc.SERIAL_CASES} == {(2, 2), (2, 5), (5, 2), (5, 5)}
    assert set(kc.B_LANES64) <= {c.B for c in kc.SERIAL_CASES}
    assert {c.rows for c in kc.SOFTPLUS_CASES} == {1, 5, 33} and set(kc.B_LANES256) <= {c.B for c in kc.SOFTPLUS_CASES}
    assert {-80.0, -40.0, -16.0, 0.0, 18.9, 19.0, 19.1, 30.0} <= set(kc.SOFTPLUS_Z)
    assert {c.rows for c in gc.ROUND_CASES} == {1, 64, 65, 130} and set(kc.B_LANES256) <= {c.B for c in gc.ROUND_CASES}


def test_the_grid_family_holds_its_conditions_and_plants_every_situation():
    """Building a problem asserts the conditions on the reference alone (exact sums, ratio == f, distance to the kink, orders on the
    1/32 grid, the exact period behind the fused launch); here: every planted situation occurs somewhere."""
    seen = {}
    for c in gc.ALLOC_CASES + gc.GROUPS_CASES:
        if c.family == "grid":
            for k, v in gc.alloc_planted(c).items():
                seen[k] = seen.get(k, False) or v
    assert all(seen.values()) and len(seen) == 4, seen
    ties = sum(int((gc.alloc_problem(c)["ref64"]["ratio"].float() == 1).sum()) for c in gc.ALLOC_CASES if c.family == "grid" and c.B == 130)
    assert ties > 0
    seen = {}
    for c in kc.DATA_DRIVEN_CASES:
        if c.family == "grid":
            for k, v in kc.data_driven_planted(c).items():
                seen[k] = seen.get(k, False) or v
    assert all(seen.values()) and len(seen) == 6, seen
    for c in gc.ALLOC_ENV_CASES:
        gc.alloc_env_problem(c)
    for c in kc.SERIAL_CASES:
        z = kc.serial_problem(c)["Z"]
        assert c.B == 1 or {40.0, -40.0, 100.0, -100.0} <= set(z.flatten().tolist()), c.id
    z = torch.cat([kc.softplus_problem(c)["Z"].flatten() for c in kc.SOFTPLUS_CASES])
    assert set(torch.tensor(kc.SOFTPLUS_Z).tolist()) <= set(z.tolist())
    x = torch.cat([gc.round_problem(c).flatten() for c in gc.ROUND_CASES])
    assert set(torch.tensor(gc.ROUND_VALUES).tolist()) <= set(x.tolist())
    assert bool(((x - 0.5) % 2 == 0).any()) and bool(((x - 0.5) % 2 == 1).any()) and bool(((x > -0.5) & (x < 0)).any())


# ---- 2. the clean restatement (and the host build of the heads) passes every case -------------------------------------------------

@pytest.mark.parametrize("name,case", ALL, ids=[f"{n}-{c.id}" for n, c in ALL])
def test_the_float32_restatement_passes(name, case):
    gc.CHECKERS[name][1](gc.TorchGlue(), case)


@pytest.fixture(scope="module")
def host():
    return kc.HostSimBackend()


# (Wn == 0, the one-store form of the data_driven head, is arithmetic of the device kernel itself: no NIC_HD body to build)
_HOST_DD = [c for c in kc.DATA_DRIVEN_CASES if c.Wn > 0]


@pytest.mark.parametrize("case", _HOST_DD, ids=[c.id for c in _HOST_DD])
def test_data_driven_head_host_build(host, case):
    kc.check_data_driven_head(host, case)


@pytest.mark.parametrize("case", kc.SERIAL_CASES, ids=[c.id for c in kc.SERIAL_CASES])
def test_serial_head_host_build(host, case):
    kc.check_serial_head_case(host, case)


@pytest.mark.parametrize("case", kc.SOFTPLUS_CASES, ids=[c.id for c in kc.SOFTPLUS_CASES])
def test_softplus_head_host_build(host, case):
    kc.check_softplus_head_case(host, case)


def test_report_the_referee_ratios():
    """(pytest -s) the worst max|kernel - fp64| / max|torch fp32 - fp64| per backend, kernel and tensor of this session"""
    for (backend, kernel, tensor), ratio in sorted(kc.REFEREE_FIGURES.items()):
        print(f"worst referee ratio  {backend:15s} {kernel:28s} {tensor:14s} {ratio:6.2f}")


# ---- 3. every class of error is noticed --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("defect", sorted(gc.DEFECTS))
def test_every_defect_fails_at_least_one_case(defect):
    caught = []
    for name in gc.DEFECTS[defect]:
        cases, check = gc.CHECKERS[name]
        for case in cases:
            try:
                check(gc.TorchGlue(defect), case)
            except AssertionError:
                caught.append(f"{name}:{case.id}")
    print(f"{defect}: caught by {len(caught)} cases: {' '.join(caught)}")
    assert caught, f"no case of {gc.DEFECTS[defect]} notices the defect {defect}"
    for name in gc.DEFECTS[defect]:      # ... by every checker that is meant to
        assert any(x.startswith(name + ":") for x in caught), f"{defect}: none of the {name} cases notices it (caught by: {caught})"
