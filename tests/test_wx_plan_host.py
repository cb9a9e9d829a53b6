"""The forward / input-gradient launch plan (csrc/wx_plan.h) without a GPU: the header is plain C++, compiled here with the host
compiler (tests/wx_plan_harness.cpp) and called on arrays of cases.  The plans are held to a table recorded from the dispatch
BEFORE it moved into the header (tests/golden/wx_plan_cu256.txt, see tools/record_wx_pins.py; 256 compute units), to the
invariants the kernels rest on at four compute-unit counts, and to the kernel names an MI355X reported at the commit before
(tests/golden/wx_dispatch_pins.json)."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import record_wx_pins as rec  # noqa: E402
from test_wgrad_plan_host import _host_clang  # noqa: E402

TABLE = os.path.join(ROOT, "tests", "golden", "wx_plan_cu256.txt")
PINS = os.path.join(ROOT, "tests", "golden", "wx_dispatch_pins.json")
# WxKernel, in the enum's order
STREAM_1x2, STREAM_1x4, DMA_128x128, DMA_64x128, DMA_32x128, STAGED_128x128, STAGED_64x128, STAGED_32x256, PRODUCT_END = range(9)
STREAM_1x1, STREAM_2x1, STREAM_2x2, STREAM_2x4, DMA_256x256, KERNEL_END = range(8, 14)
STREAM, DMA, STAGED = 0, 1, 2   # WxFamily
FIELDS = ("kernel", "grid", "family", "bm", "bn", "threads")
CUS = (64, 104, 256, 304)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("wx_plan") / "harness.so")
    # (-Wall -Werror: the header has to stay clean C++ for a compiler that knows nothing of HIP)
    subprocess.run([_host_clang(), "-O2", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", "-o", so,
                    os.path.join(ROOT, "tests", "wx_plan_harness.cpp")], check=True)
    lib = ctypes.CDLL(so)
    lib.nic_test_wx_plans.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]
    lib.nic_test_wx_kernel_name.argtypes = [ctypes.c_int, ctypes.c_char_p]
    lib.nic_test_wx_kernel_name.restype = ctypes.c_char_p
    lib.nic_test_wx_operands.argtypes = [ctypes.c_uint64, ctypes.c_int64, ctypes.c_int64, ctypes.c_int, ctypes.c_int]
    lib.nic_test_bf16_wx_tile.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    assert (lib.nic_test_wx_product_end(), lib.nic_test_wx_kernel_end()) == (PRODUCT_END, KERNEL_END)
    return lib


@pytest.fixture(scope="module")
def table():
    """rows of (M, K, ncols, operands_ok, kernel name without the epilogue, grid, block)"""
    with open(TABLE) as f:
        rows = [ln.split() for ln in f if not ln.startswith("#")]
    assert len(rows) <= 4096 and [tuple(map(int, r[:4])) for r in rows] == rec.plan_grid()
    return rows


def _plans(harness, cases, cus=256, stream=-1, tile=-1):
    """cases: rows of (M, K, ncols, operands_ok) -> {field: array}"""
    cases = np.asarray(cases, dtype=np.int32)
    n = len(cases)
    full = np.ascontiguousarray(np.column_stack([cases, np.full(n, cus), np.full(n, stream), np.full(n, tile)]), dtype=np.int32)
    out = np.empty((n, len(FIELDS)), dtype=np.int32)
    harness.nic_test_wx_plans(full.ctypes.data, out.ctypes.data, n)
    return {f: out[:, i].astype(np.int64) for i, f in enumerate(FIELDS)}


def _name(harness, kernel, epi="EPI_BIAS_ACT"):
    return harness.nic_test_wx_kernel_name(int(kernel), epi.encode()).decode()


def test_plans_equal_the_recorded_table(harness, table):
    p = _plans(harness, [r[:4] for r in table])
    got = [(_name(harness, k, "").replace(",>", ">"), int(g), int(t)) for k, g, t in zip(p["kernel"], p["grid"], p["threads"])]
    want = [(r[4], int(r[5]), int(r[6])) for r in table]
    bad = [i for i in range(len(table)) if got[i] != want[i]]
    assert not bad, [(table[i][:4], got[i], want[i]) for i in bad[:8]]
    assert {w[0] for w in want} == {_name(harness, k, "").replace(",>", ">") for k in range(PRODUCT_END)}   # every product kernel comes up


def _ceil(a, b):
    return -(-a // b)


@pytest.mark.parametrize("cus", CUS)
def test_plan_invariants_over_the_grid(harness, cus):
    """derived from the kernels, not from the pickers"""
    cases = np.array(rec.plan_grid(), dtype=np.int64)
    M, K, ncols, ok = cases.T
    p = _plans(harness, cases, cus)
    k, fam = p["kernel"], p["family"]

    def holds(cond, what):
        bad = np.flatnonzero(~cond)
        assert bad.size == 0, (what, cus, [(tuple(cases[i]), {f: int(p[f][i]) for f in FIELDS}) for i in bad[:4]])

    holds(k < PRODUCT_END, "no tuning-only kernel without a WxForce (streamed <1,1> among them: unreachable)")
    holds(p["grid"] == _ceil(M, p["bm"]) * _ceil(ncols, p["bn"]), "one workgroup per block of the output")
    # buffer descriptors of the streamed and LDS-DMA kernels: 16-byte alignment, lda % 4 == 0, fewer than 2^28 floats
    holds((fam == STAGED) == (ok == 0), "register-staged kernels if and only if the operands are not eligible")
    staged = np.where(M > 64, STAGED_128x128, np.where(M > 32, STAGED_64x128, STAGED_32x256))
    holds((fam != STAGED) | (k == staged), "register-staged tile by M > 64, 33..64, <= 32")
    tiles32 = _ceil(M, 32) * _ceil(ncols, 32)
    ks = np.where(k == STREAM_1x2, 2, 4)
    holds((fam != STREAM) | ((k == STREAM_1x2) | (k == STREAM_1x4)), "streamed: KS in {2, 4}")
    holds((fam != STREAM) | ((K >= 128) & (tiles32 <= 4 * cus)), "streamed: K >= 128, at most 4 tiles of 32 x 32 per CU")
    holds((fam != STREAM) | (K >= 64 * ks), "streamed: every wavefront owns at least one full block of four k groups")
    holds((fam != STREAM) | (tiles32 * ks <= 8 * cus), "streamed: at most 8 wavefronts per CU")
    holds((fam != STREAM) | (p["threads"] == 64 * ks), "streamed: KS wavefronts per workgroup")
    holds((k != DMA_128x128) | (_ceil(M, 128) * _ceil(ncols, 128) >= 2 * cus), "LDS-DMA 128 x 128: two workgroups per CU")
    holds((fam != DMA) | (M > 32) | (k == DMA_32x128), "LDS-DMA, M <= 32: 32 x 128")
    default = [harness.nic_test_wx_plan_unforced(*map(int, c), cus) for c in cases[::7]]
    assert default == k[::7].tolist()   # WxForce defaults to nothing forced


@pytest.mark.parametrize("cus", (104, 256))
def test_a_force_is_honoured_where_the_ladder_before_honoured_it(harness, cus):
    """NIC_WX_STREAM = 10 NT + KS: that streamed kernel, any other value: never streamed; NIC_WX_TILE 0..3 (tune bit 128 = 3): that
    LDS-DMA tiling where the launch is not streamed, any other value: ignored; operands off the fast path: never forced"""
    cases = np.array(rec.plan_grid(), dtype=np.int64)
    ok = cases[:, 3] == 1
    free = _plans(harness, cases, cus)["kernel"]
    streams = {11: STREAM_1x1, 12: STREAM_1x2, 14: STREAM_1x4, 21: STREAM_2x1, 22: STREAM_2x2, 24: STREAM_2x4}
    tiles = {0: DMA_128x128, 1: DMA_64x128, 2: DMA_32x128, 3: DMA_256x256}
    never = _plans(harness, cases, cus, stream=0)["kernel"]   # the LDS-DMA picker's choice for every eligible launch
    assert ((never == free) | (free <= STREAM_1x4)).all()
    assert np.isin(never[ok], (DMA_128x128, DMA_64x128, DMA_32x128)).all()
    for stream in (-1, 0, 13, 10, 11, 12, 14, 21, 22, 24):
        for tile in (-1, 0, 1, 2, 3, 4, 7):
            p = _plans(harness, cases, cus, stream, tile)
            not_streamed = never if stream >= 0 else free
            if tile in tiles:
                not_streamed = np.where(np.isin(not_streamed, (DMA_128x128, DMA_64x128, DMA_32x128)), tiles[tile], not_streamed)
            want = np.where(ok, streams[stream] if stream in streams else not_streamed, free)
            assert (p["kernel"] == want).all(), (stream, tile)
            assert (p["grid"] == _ceil(cases[:, 0], p["bm"]) * _ceil(cases[:, 2], p["bn"])).all()


def test_operand_eligibility(harness):
    ok = lambda **kw: harness.nic_test_wx_operands(*[{**dict(ab=0x7f0000001000, lda=512, ldb=1024, M=512, K=512), **kw}[k]
                                                     for k in ("ab", "lda", "ldb", "M", "K")])
    assert ok() == 1
    assert ok(ab=0x7f0000001004) == 0 and ok(lda=51) == 0 and ok(ldb=1022) == 0   # off a 16-byte boundary, ragged row strides
    assert ok(lda=1 << 19) == 0 and ok(lda=(1 << 19) - 4) == 1                    # M * lda = 2^28 floats: past the buffer range
    assert ok(ldb=1 << 19) == 0 and ok(ldb=(1 << 19) - 4) == 1                    # K * ldb likewise
    assert ok(lda=1 << 19, M=511) == 1 and ok(ldb=1 << 19, K=511) == 1


def test_bf16_tile_on_both_sides_of_two_tiles_per_cu(harness):
    def tile(M, ncols, cus):
        out = (ctypes.c_int64 * 2)()
        harness.nic_test_bf16_wx_tile(M, ncols, cus, out)
        return tuple(out)
    assert tile(512, 16384, 256) == (2, 512)            # 4 x 128 tiles of 128 x 128 = 2 per CU
    assert tile(512, 16384 - 128, 256) == (1, 8 * 254)  # 508: 64 x 64 tiles
    assert tile(512, 16384 - 127, 256) == (2, 512)      # a partial column tile counts
    assert tile(512, 16384, 304) == (1, 8 * 256) and tile(128, 26 * 128, 13) == (2, 26) and tile(129, 12 * 128, 13) == (1, 3 * 24)


def test_kernel_names(harness):
    want = {STREAM_1x2: "gemm_wx_stream_kernel<1,2,%s>", STREAM_1x4: "gemm_wx_stream_kernel<1,4,%s>",
            DMA_128x128: "gemm_wx_dma_kernel<2,4,2,1,%s>", DMA_64x128: "gemm_wx_dma_kernel<2,4,1,1,%s>",
            DMA_32x128: "gemm_wx_dma_kernel<1,4,1,1,%s>", STAGED_128x128: "gemm_wx_kernel<2,2,2,2,%s>",
            STAGED_64x128: "gemm_wx_kernel<1,4,2,1,%s>", STAGED_32x256: "gemm_wx_kernel<1,4,1,2,%s>"}
    assert sorted(want) == list(range(PRODUCT_END))
    for kernel, fmt in want.items():
        for epi in ("EPI_BIAS_ACT", "EPI_DGRAD"):
            assert _name(harness, kernel, epi) == fmt % epi
    assert _name(harness, STREAM_1x1, "EPI_DGRAD") == "gemm_wx_stream_kernel<1,1,EPI_DGRAD>"
    assert _name(harness, DMA_256x256) == "gemm_wx_dma_kernel<2,4,4,2,EPI_BIAS_ACT>"


def test_the_plan_names_the_kernel_the_gpu_recorded(harness):
    """ties the table (recorded from a copy of the dispatch) to what the library before really launched on 256 compute units"""
    with open(PINS) as f:
        pins = json.load(f)
    assert sorted(pins) == sorted(rec.PIN_IDS)
    for case_id, direction in rec.PIN_RUNS:
        case = next(c for c in rec.PIN_CASES if c[0] == case_id)
        _, M, K, B, _ = case
        p = _plans(harness, [(M, K, (B + 3) // 4 * 4, int(rec.case_operands_ok(case)))])
        epi = "EPI_BIAS_ACT" if direction == "fwd" else "EPI_DGRAD"
        assert _name(harness, p["kernel"][0], epi) == pins[f"{case_id}-{direction}"]["kernel"], (case_id, direction)
