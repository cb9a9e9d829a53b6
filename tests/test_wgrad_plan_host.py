"""The weight-gradient launch plan (csrc/wgrad_plan.h) without a GPU: the header is plain C++, compiled here with the host
compiler (tests/wgrad_plan_harness.cpp) and called on arrays of cases.  The recommended slot counts are held to a table recorded
from the library BEFORE the plan moved into the header (tools/record_wgrad_pins.py --slots, 256 compute units); the plans are
held to the invariants the kernels' correctness rests on."""
import ctypes
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import record_wgrad_pins as rec  # noqa: E402
from neural_inventory_control_amd import build  # noqa: E402

SLOT_TABLE = os.path.join(ROOT, "tests", "golden", "wgrad_slots_cu256.txt")
GRID_TS = rec.SLOT_TS[:4]   # 1, 2, 7, 100
SMALL, DMA, STAGED = 0, 1, 2                   # WgradFamily
ONE_LAUNCH, PER_PERIOD, PER_GROUP = 0, 1, 2    # WgradCut
RAW = ("tile", "tile_single", "slots", "chunk", "wg_scen_splits", "wg_ppg", "flush", "cut", "launch_periods", "launches", "covered",
       "small_single", "small_many")
FIELDS = RAW + ("family", "family_single", "slot_pairs", "scen_splits", "groups", "ppg")


def _host_clang():
    hipcc = os.path.realpath(shutil.which(build._hipcc()) or build._hipcc())
    for c in (os.path.join(os.path.dirname(hipcc), "..", "llvm", "bin", "clang++"), "/opt/rocm/llvm/bin/clang++",
              shutil.which("clang++")):
        if c and os.path.isfile(c):
            return c
    raise RuntimeError("no clang++ to build the host harness of csrc/wgrad_plan.h")


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("wgrad_plan") / "harness.so")
    # (-Wall -Werror: the header has to stay clean C++ for a compiler that knows nothing of HIP)
    subprocess.run([_host_clang(), "-O2", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", "-o", so,
                    os.path.join(ROOT, "tests", "wgrad_plan_harness.cpp")], check=True)
    lib = ctypes.CDLL(so)
    lib.nic_test_wgrad_slots.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    lib.nic_test_wgrad_plans.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]
    lib.nic_test_wgrad_tile_name.argtypes = [ctypes.c_int]
    lib.nic_test_wgrad_tile_name.restype = ctypes.c_char_p
    lib.nic_test_wgrad_operands.argtypes = [ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int64, ctypes.c_int64, ctypes.c_int, ctypes.c_int]
    return lib


@pytest.fixture(scope="module")
def table():
    """rows of N K B single-period-slots + the all-period slots for every T of rec.SLOT_TS"""
    t = np.loadtxt(SLOT_TABLE, dtype=np.int64, comments="#")
    assert t.shape == (len(rec.slot_grid()), 4 + len(rec.SLOT_TS)) and t.shape[0] <= 4096
    assert [tuple(r) for r in t[:, :3]] == rec.slot_grid()
    return t


def _slots(harness, cases, cus=256):
    cases = np.ascontiguousarray(cases, dtype=np.int32)
    out = np.empty((len(cases), 2), dtype=np.int32)
    harness.nic_test_wgrad_slots(cases.ctypes.data, out.ctypes.data, len(cases), cus)
    return out


def _plans(harness, cases):
    """cases: rows of (entry, N, K, B, T, slots given, buffer-eligible, DMA-eligible) -> {field: array}: the plan's fields and
    what the harness counted over its launches (RAW), plus the slot factors behind the WgParams encoding (scen_splits = 0: every
    slot a scenario split of all the periods of a launch)"""
    cases = np.ascontiguousarray(cases, dtype=np.int32)
    out = np.empty((len(cases), len(RAW)), dtype=np.int32)
    harness.nic_test_wgrad_plans(cases.ctypes.data, out.ctypes.data, len(cases))
    p = {f: out[:, i].astype(np.int64) for i, f in enumerate(RAW)}
    for f, t in (("family", p["tile"]), ("family_single", p["tile_single"])):
        p[f] = np.where(t <= 3, SMALL, np.where(t <= 10, DMA, STAGED))   # WgradTile: 4 small, 7 LDS-DMA, 4 register-staged
    p["slot_pairs"] = (p["wg_scen_splits"] > 0).astype(np.int64)
    p["scen_splits"] = np.where(p["slot_pairs"] == 1, p["wg_scen_splits"], p["slots"])
    p["groups"] = p["slots"] // np.maximum(p["scen_splits"], 1)
    p["ppg"] = np.where(p["slot_pairs"] == 1, p["wg_ppg"], np.minimum(p["launch_periods"], cases[:, 4]))
    return p


def test_recommended_slots_equal_the_recorded_table(harness, table):
    for j, T in enumerate(rec.SLOT_TS):
        cases = np.column_stack([table[:, :3], np.full(len(table), T)])
        got = _slots(harness, cases)
        bad = np.flatnonzero((got[:, 0] != table[:, 3]) | (got[:, 1] != table[:, 4 + j]))
        assert bad.size == 0, [(tuple(cases[i]), tuple(got[i]), (int(table[i, 3]), int(table[i, 4 + j]))) for i in bad[:8]]


def test_recommended_slots_of_degenerate_arguments(harness):
    assert (_slots(harness, [(0, 4, 100, 1), (4, 0, 100, 1), (4, 4, 0, 1), (-1, 4, 100, 1)]) == 0).all()
    assert _slots(harness, [(64, 64, 100, 0)]).tolist() == [[_slots(harness, [(64, 64, 100, 1)])[0, 0], 0]]


def _dma_shape(N, K):   # wgrad_dma_shape restated (as tests/test_gpu_kernels.py does)
    return ((N >= 192) & (K >= 65)) | ((N >= 384) & (K <= 64)) | ((96 <= N) & (N <= 128) & (K >= 192))


def test_plan_invariants_over_the_grid(harness, table):
    """every grid row x T x slots given in {1, 3, 7, 64, recommended} x operand eligibility x both entry points"""
    rows = []
    for j, T in enumerate(GRID_TS):
        for given in (1, 3, 7, 64, None):
            for entry in (0, 1):
                if entry == 0 and T != 1:
                    continue
                rec_slots = table[:, 3] if entry == 0 else table[:, 4 + j]
                slots = rec_slots if given is None else np.full(len(table), given)
                for buffer_ok, dma_ok in ((1, 1), (1, 0), (0, 0)):
                    n = len(table)
                    rows.append(np.column_stack([np.full(n, entry), table[:, :3], np.full(n, T), slots, np.full(n, buffer_ok),
                                                 np.full(n, dma_ok)]))
    cases = np.concatenate(rows)
    entry, N, K, B, T, given, buffer_ok, dma_ok = cases.T
    p = _plans(harness, cases)

    def holds(cond, what):
        bad = np.flatnonzero(~cond)
        assert bad.size == 0, (what, [(tuple(cases[i]), {f: int(p[f][i]) for f in FIELDS}) for i in bad[:4]])

    holds((p["slots"] >= 1) & (p["slots"] <= given), "slots addressed <= slots given")
    holds(p["scen_splits"] * p["groups"] == p["slots"], "slots = scenario splits x period groups")
    holds((p["chunk"] % 32 == 0) & (p["chunk"] > 0), "chunk % 32 == 0")
    holds(p["scen_splits"] * p["chunk"] >= B, "the scenario splits cover the scenarios")
    holds(p["groups"] * p["ppg"] >= np.minimum(p["launch_periods"], T), "the period groups cover the periods of a launch")
    holds((p["slot_pairs"] == 1) | (p["wg_ppg"] == 0), "scen_splits = periods_per_group = 0 together")
    holds(p["slot_pairs"].astype(bool) | (p["groups"] == 1), "without (group, split) slots there is one group")
    # the launches wgrad_launch enumerates: consecutive, [0, T) exactly once
    holds((p["covered"] == T) & (p["launches"] == -(-T // p["launch_periods"])), "the launches cover the periods exactly once")
    holds((p["cut"] != ONE_LAUNCH) | (p["launch_periods"] >= T), "one launch holds the whole horizon")
    holds((p["cut"] != PER_PERIOD) | (p["launch_periods"] == 1), "a launch per period")
    holds((entry == 1) | (p["cut"] == ONE_LAUNCH), "nic_linear_wgrad is one launch")
    # kernel families
    dma = (p["family"] == DMA) | (p["family_single"] == DMA)
    holds(~dma | ((dma_ok == 1) & (B % 32 == 0) & _dma_shape(N, K)), "LDS-DMA only for eligible operands, B % 32 == 0, DMA shapes")
    holds(~dma | ((p["tile"] == p["tile_single"]) & (p["cut"] == ONE_LAUNCH)), "LDS-DMA: one launch, one kernel")
    holds(p["small_many"] == 0, "wgrad_small_kernel only in launches of one period")
    small = (p["family"] == SMALL) | (p["family_single"] == SMALL)
    holds(~small | ((N <= 32) & (K <= 128) & (buffer_ok == 1) & ~p["slot_pairs"].astype(bool)), "wgrad_small_kernel: N <= 32, K <= 128")
    # no accumulator sums more than ~8k terms (chunk x periods) before it goes to the slab
    pairs = p["slot_pairs"] == 1
    holds((p["family"] != DMA) | (entry == 0) | (p["flush"] == np.maximum(1, 8192 // p["chunk"])), "LDS-DMA flush interval")
    holds(~(pairs & (p["family"] == STAGED)) | ((p["groups"] > 1) & (p["chunk"] * p["ppg"] <= 8192)), "(group, split) slots, staged")
    holds((p["cut"] != PER_GROUP) | (p["launch_periods"] == np.maximum(1, 8192 // -(-B // given))), "periods per launch")
    holds((p["flush"] > 0) == ((p["family"] == DMA) & (entry == 1)), "only the all-period LDS-DMA launch flushes")


# (N, K, B, T, slots) of test_linear_wgrad_periods_splits_the_horizon_into_period_groups with the kernel it expects, and the tile
PERIOD_GROUP_CASES = [
    (512, 512, 1024, 7, None, "dma_big"), (512, 512, 256, 9, 64, "dma_big"), (512, 51, 1024, 6, None, "dma_tall"),
    (512, 51, 512, 5, 7, "dma_tall"), (98, 512, 512, 5, None, "dma_mid"), (512, 393, 384, 4, 6, "dma_wide7"),
    (512, 512, 8192, 3, None, "dma_big"), (512, 66, 1024, 6, None, "dma_half"), (320, 150, 512, 5, None, "dma_big"),
    (64, 597, 72, 19, None, "staged_64x128"), (66, 64, 72, 10, None, "staged_128x128"), (64, 64, 100, 7, 5, "staged_64x128"),
    (200, 100, 300, 6, None, "staged_128x128")]


@pytest.mark.parametrize("N,K,B,T,slots,tile", PERIOD_GROUP_CASES)
def test_kernel_and_tile_of_the_period_group_cases(harness, N, K, B, T, slots, tile):
    given = slots or int(_slots(harness, [(N, K, B, T)])[0, 1])
    p = _plans(harness, [(1, N, K, B, T, given, 1, 1)])
    dma = B % 32 == 0 and bool(_dma_shape(np.int64(N), np.int64(K)))
    assert int(p["family"][0]) == (DMA if dma else STAGED)
    assert tile.startswith("dma" if dma else "staged")
    assert harness.nic_test_wgrad_tile_name(int(p["tile"][0])).decode() == tile
    assert int(p["cut"][0]) == ONE_LAUNCH and int(p["slot_pairs"][0]) == 1 and 1 <= int(p["slots"][0]) <= given


def test_the_three_cuts_of_the_register_staged_horizon(harness):
    """off the LDS-DMA path: a launch per period (tiny layers, T = 1), one launch over (group, split) slots, a launch per <= 8k-term
    group of periods - with the small kernel for a left-over single period"""
    cases = [(1, 32, 4, 100, 3, 4, 1, 1), (1, 200, 100, 300, 1, 2, 1, 1), (1, 64, 64, 72, 10, 64, 1, 1),
             (1, 66, 64, 2000, 7, 1, 1, 1), (1, 17, 96, 2048, 5, 1, 1, 1), (1, 17, 96, 2048, 5, 1, 0, 0)]
    p = _plans(harness, cases)
    name = [harness.nic_test_wgrad_tile_name(int(t)).decode() for t in p["tile"]]
    single = [harness.nic_test_wgrad_tile_name(int(t)).decode() for t in p["tile_single"]]
    assert p["cut"].tolist() == [PER_PERIOD, PER_PERIOD, ONE_LAUNCH, PER_GROUP, PER_GROUP, PER_GROUP]
    assert p["launch_periods"].tolist() == [1, 1, 10, 4, 4, 4]
    assert name == ["small<1>", "staged_128x128", "staged_64x128", "staged_128x128", "staged_32x256", "staged_32x256"]
    assert single == ["small<1>", "staged_128x128", "staged_64x128", "staged_128x128", "small<3>", "staged_32x256"]
    assert (int(p["scen_splits"][2]), int(p["groups"][2]), int(p["chunk"][2]), int(p["ppg"][2])) == (1, 10, 96, 1)


def test_operand_eligibility(harness):
    ok = lambda **kw: harness.nic_test_wgrad_operands(*[{**dict(dyx=0x7f0000001000, slab=0x7f0000002000, ldb=1024, lds=516,
                                                                N=512, K=512), **kw}[k] for k in ("dyx", "slab", "ldb", "lds", "N", "K")])
    assert ok() == 3
    assert ok(dyx=0x7f0000001004) == 0 and ok(ldb=1022) == 0          # dY / X off a 16-byte boundary, ragged row stride
    assert ok(ldb=1 << 19) == 0 and ok(ldb=(1 << 19) - 4) == 3         # 512 rows x 2^19 = 2^28 floats: past the buffer range
    assert ok(ldb=1 << 19, N=511, K=511) == 3 and ok(ldb=1 << 19, N=511) == 0
    assert ok(slab=0x7f0000002008) == 1 and ok(lds=513) == 1           # the slab's alignment only matters to the LDS-DMA kernel
