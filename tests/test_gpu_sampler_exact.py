"""csrc/sampler.hip draw for draw against the host Philox reference (tests/philox_reference.py).

The sampler promises that every number is a pure function of (seed, global scenario index, period, variate).  Here that function
is computed on the host in float64 for every element the test compares, and each kernel of the sampler has to land inside the
reference's band (normal demands) or inside the accepted interval of integers (Poisson) - no statistics, no self-consistency.
Every output buffer is pre-filled with NaN, has a leading dimension larger than the batch and guard zones on both sides;
whatever lies outside (t < T, s < S, b < B) must still be that NaN afterwards, bit for bit.  Run with -s for the largest
|gpu - reference| / band ratio of every kernel (recorded in DESIGN.md, sampler row a1).
"""
import copy
import functools
from collections import defaultdict

import numpy as np
import pytest
import torch

import philox_reference as pr
from neural_inventory_control_amd import _lib, ops
from neural_inventory_control_amd._lib import NicError

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = 64                       # floats of NaN in front of and behind every output buffer (a multiple of four: 16-byte alignment)
SEED_A, SEED_B = 1234, 0x9E3779B97F4A7C15     # (the second has a non-zero high key word)


def _last_kernel():
    return _lib.lib().nic_last_kernel().decode()


def _nan_out(T, S, ldb, shift=0):
    """A [T][S][ldb] view into a NaN-filled buffer with guard zones; `shift` floats move its base off the 16-byte grid."""
    buf = torch.full((GUARD + shift + T * S * ldb + GUARD,), float("nan"), device=DEV)
    out = buf[GUARD + shift: GUARD + shift + T * S * ldb].view(T, S, ldb)
    assert out.stride(1) == ldb and out.data_ptr() == buf.data_ptr() + 4 * (GUARD + shift)
    return buf, out


def _read_back(buf, T, S, ldb, B, shift=0):
    """The written block [T][S][B] as float64, after asserting that every other float of the buffer is the untouched NaN."""
    torch.cuda.synchronize()
    h = buf.cpu()
    inner = h[GUARD + shift: GUARD + shift + T * S * ldb].view(T, S, ldb)
    got = inner[:, :, :B].clone()
    inner[:, :, :B] = float("nan")
    nan_bits = torch.full((1,), float("nan")).view(torch.int32)
    touched = int((h.view(torch.int32) != nan_bits).sum())
    assert touched == 0, f"{touched} floats written outside (t < {T}, s < {S}, b < {B})"
    return got.double().numpy()


def _in_band(kernel, got, want, band, where=""):
    """Every element inside the band; prints the worst ratio (the number DESIGN.md records)."""
    assert got.shape == want.shape == band.shape, (got.shape, want.shape)
    assert np.isfinite(got).all(), f"{kernel}: {int((~np.isfinite(got)).sum())} elements not written"
    ratio = np.abs(got - want) / band
    worst = float(ratio.max())
    print(f"[sampler exact] {kernel} {where}: worst |gpu - reference| / band = {worst:.3f} over {ratio.size} elements")
    bad = np.argwhere(ratio > 1.0)
    assert bad.size == 0, (f"{kernel} {where}: {len(bad)} elements outside the band, first (t, s, b, gpu, reference, band): "
                           + str([(tuple(i), got[tuple(i)], want[tuple(i)], band[tuple(i)]) for i in bad[:5]]))
    return worst


def _dev(a):
    return torch.as_tensor(np.asarray(a, dtype=np.float32)).to(DEV)


def _normal_params(S, clip, seed):
    """std in [0.5, 2.5); with clipping the means sit at 0.43 std, so that about a third of the draws clip."""
    rng = np.random.default_rng(1000 + S + seed % 97)
    std = (0.5 + 2.0 * rng.random(S)).astype(np.float32)
    mean = (0.43 * std if clip else 3.0 + 5.0 * rng.random(S)).astype(np.float32)
    return mean, std


# ---- sample_equicorrelated_kernel<1> ------------------------------------------------------------------------------------------

_EQ_S, _EQ_T = (2, 3, 4, 5, 16, 33), (1, 4, 5, 9)
_EQ_BATCH = ((1, 0), (63, 3), (257, 2 ** 40 + 1), (300, 2 ** 32 - 100), (300, 0), (257, 3), (63, 2 ** 40 + 1), (300, 3))
_EQ_RHO = (0.0, 0.3, 1.0)


def _eq_cases():
    cases = []
    for i, (S, T) in enumerate((S, T) for S in _EQ_S for T in _EQ_T):
        B, off = _EQ_BATCH[i % len(_EQ_BATCH)]
        cases.append((S, T, B, off, _EQ_RHO[(i + i // 3) % 3], (i // 2) % 2 == 0, (SEED_A, SEED_B)[(i // 5 + i) % 2]))
    return cases


def test_equicorrelated_cases_cover_what_they_should():
    c = _eq_cases()
    assert {x[0] for x in c} == set(_EQ_S) and {x[1] for x in c} == set(_EQ_T)
    assert {x[2] for x in c} == {1, 63, 257, 300} and {x[3] for x in c} == {0, 3, 2 ** 32 - 100, 2 ** 40 + 1}
    assert (300, 2 ** 32 - 100) in {(x[2], x[3]) for x in c}      # the batch straddles the carry into the second counter word
    assert {(x[4], x[5]) for x in c} == {(r, k) for r in _EQ_RHO for k in (True, False)}
    assert {(x[6], x[3]) for x in c} >= {(s, o) for s in (SEED_A, SEED_B) for o in (0, 2 ** 32 - 100)}


@pytest.mark.parametrize("S,T,B,off,rho,clip,seed", _eq_cases())
def test_equicorrelated_one_period_per_lane(S, T, B, off, rho, clip, seed):
    mean, std = _normal_params(S, clip, seed)
    ldb = B + 5
    buf, out = _nan_out(T, S, ldb)
    ops.sample_demand_equicorrelated(out, T, S, B, off, seed, _dev(mean), _dev(std), rho, clip)
    assert _last_kernel() == "sample_equicorrelated_kernel<1>"
    got = _read_back(buf, T, S, ldb, B)
    want, band = pr.equicorrelated(seed, off + np.arange(B), T, mean, std, rho, clip)
    _in_band("sample_equicorrelated_kernel<1>", got, want, band, f"S={S} T={T} B={B} off={off} rho={rho} clip={clip}")
    if clip and B >= 63:
        assert got.min() == 0.0 and 0.2 < float((got == 0.0).mean()) < 0.47      # about a third of the draws clip


@pytest.mark.parametrize("clip", [False, True])
def test_one_store_through_the_general_kernel_when_the_base_is_not_16_byte_aligned(clip):
    """S = 1 through a view whose base pointer is offset by one float: the general kernel, not the one-store kernel - and the
    one store then has a common factor, with rho acting on nothing but the split of its variance."""
    T, B, off, rho = 5, 257, 3, 0.3
    mean, std = _normal_params(1, clip, 7)
    ldb = 264
    buf, out = _nan_out(T, 1, ldb, shift=1)
    assert out.data_ptr() % 16 == 4
    ops.sample_demand_equicorrelated(out, T, 1, B, off, SEED_B, _dev(mean), _dev(std), rho, clip)
    assert _last_kernel() == "sample_equicorrelated_kernel<1>"
    got = _read_back(buf, T, 1, ldb, B, shift=1)
    want, band = pr.equicorrelated(SEED_B, off + np.arange(B), T, mean, std, rho, clip)
    _in_band("sample_equicorrelated_kernel<1>", got, want, band, f"S=1 misaligned clip={clip}")


# ---- sample_equicorrelated_kernel<4> ------------------------------------------------------------------------------------------

def test_equicorrelated_four_periods_per_lane():
    """Over the 4 Mi (scenario, period) threshold with a ragged horizon and a ragged batch; scenarios 0-299, the last 300 and 300
    random ones are compared over every period and store."""
    S, T, B, off, rho, clip = 2, 17, 262147, 2 ** 32 - 200000, 0.3, True
    assert B * T >= 4 << 20 and T % 4 and B % 256
    mean, std = _normal_params(S, clip, 11)
    ldb = B + 5
    buf, out = _nan_out(T, S, ldb)
    ops.sample_demand_equicorrelated(out, T, S, B, off, SEED_B, _dev(mean), _dev(std), rho, clip)
    assert _last_kernel() == "sample_equicorrelated_kernel<4>"
    got = _read_back(buf, T, S, ldb, B)
    pick = np.concatenate([np.arange(300), np.arange(B - 300, B),
                           np.sort(np.random.default_rng(5).choice(np.arange(300, B - 300), 300, replace=False))])
    want, band = pr.equicorrelated(SEED_B, off + pick, T, mean, std, rho, clip)
    _in_band("sample_equicorrelated_kernel<4>", got[:, :, pick], want, band, f"S={S} T={T} B={B}")
    assert np.isfinite(got).all()


# ---- sample_one_store_kernel ---------------------------------------------------------------------------------------------------

_ONE_OFFSETS = (0, 1, 6, 2 ** 32 - 2)     # (at 2^32 - 2 the carry falls inside one lane's four scenarios)


@pytest.mark.parametrize("T", [1, 3, 4, 7])
@pytest.mark.parametrize("B", [1, 2, 3, 5, 1023, 2001])
def test_one_store(T, B):
    i = (1, 3, 4, 7).index(T) + (1, 2, 3, 5, 1023, 2001).index(B)
    off, clip, seed = _ONE_OFFSETS[i % 4], (i // 2) % 2 == 0, (SEED_A, SEED_B)[i % 2]
    mean, std = _normal_params(1, clip, seed + T)
    ldb = (B + 3) // 4 * 4 + 4
    buf, out = _nan_out(T, 1, ldb)
    ops.sample_demand_equicorrelated(out, T, 1, B, off, seed, _dev(mean), _dev(std), 0.3, clip)
    assert _last_kernel() == "sample_one_store_kernel"
    got = _read_back(buf, T, 1, ldb, B)
    want, band = pr.one_store(seed, off + np.arange(B), T, mean, std, clip)
    _in_band("sample_one_store_kernel", got, want, band, f"T={T} B={B} off={off} clip={clip}")


@pytest.mark.parametrize("off", _ONE_OFFSETS)
@pytest.mark.parametrize("clip", [False, True])
def test_one_store_at_every_offset(off, clip):
    T, B = 7, 1023
    mean, std = _normal_params(1, clip, 3)
    ldb = 1028
    buf, out = _nan_out(T, 1, ldb)
    ops.sample_demand_equicorrelated(out, T, 1, B, off, SEED_B, _dev(mean), _dev(std), 0.0, clip)
    assert _last_kernel() == "sample_one_store_kernel"
    got = _read_back(buf, T, 1, ldb, B)
    want, band = pr.one_store(SEED_B, off + np.arange(B), T, mean, std, clip)
    _in_band("sample_one_store_kernel", got, want, band, f"T={T} B={B} off={off} clip={clip}")
    if clip:
        assert 0.2 < float((got == 0.0).mean()) < 0.47


# ---- sample_cholesky_kernel<SMAX> ---------------------------------------------------------------------------------------------

def _factor(S):
    """Dense lower factor of a random SPD matrix with negative correlations."""
    rng = np.random.default_rng(200 + S)
    A = rng.standard_normal((S, S)) * 0.4
    cov = A @ A.T + np.eye(S)
    assert S == 1 or (cov < 0).any()
    return np.linalg.cholesky(cov).astype(np.float32)


@pytest.mark.parametrize("S", [1, 4, 5, 16, 17, 32, 33, 64, 65, 96])
def test_general_covariance(S):
    """Every instantiation at both of its edges."""
    T, B, off = 3, 130, 2 ** 32 - 65
    clip = S % 2 == 1
    L = _factor(S)
    mean = (np.linspace(0.2, 1.5, S) if clip else np.linspace(3.0, 9.0, S)).astype(np.float32)
    ldb = B + 6
    buf, out = _nan_out(T, S, ldb)
    ops.sample_demand(out, T, S, B, off, SEED_B, 0, _dev(mean), _dev(L).contiguous(), clip)
    smax = next(m for m in (4, 16, 32, 64, 96) if S <= m)
    assert _last_kernel() == f"sample_cholesky_kernel<{smax}>"
    got = _read_back(buf, T, S, ldb, B)
    want, band = pr.general_covariance(SEED_B, off + np.arange(B), T, mean, L, clip)
    _in_band(f"sample_cholesky_kernel<{smax}>", got, want, band, f"S={S} clip={clip}")


# ---- sample_poisson_kernel -----------------------------------------------------------------------------------------------------

_LAMS = (0.05, 0.7, 5.0, 12.0, 30.0)
_POISSON_CASES = {                   # name: (S, T, B, scenario offset, seed, lambda per store)
    **{f"S{S}": (S, 3, 300, 2 ** 32 - 150, SEED_A + S, [_LAMS[(s + S) % 5] for s in range(S)]) for S in (1, 2, 5, 9)},
    "S256": (256, 2, 130, 7, SEED_B, [_LAMS[s % 5] for s in range(256)]),     # a 64 KiB table
    "past_table": (2, 3, 300, 2 ** 40 + 1, SEED_B, [45.0, 80.0]),
}


@functools.lru_cache(maxsize=None)
def _poisson_reference(name):
    """The accepted intervals of a case, computed once and shared (read-only)."""
    S, T, B, off, seed, lam = _POISSON_CASES[name]
    lo, hi = pr.poisson_interval(seed, off + np.arange(B), T, lam)
    lo.setflags(write=False), hi.setflags(write=False)
    return lo, hi


def _in_interval(got, lo, hi, where):
    assert np.isfinite(got).all() and np.array_equal(got, np.round(got)), f"{where}: not every value is an integer"
    bad = np.argwhere((got < lo) | (got > hi))
    print(f"[sampler exact] sample_poisson_kernel {where}: {got.size} draws, {len(bad)} outside the accepted interval, "
          f"{int((hi > lo).sum())} intervals wider than one integer")
    assert bad.size == 0, (f"{where}: {len(bad)} draws outside the accepted interval, first (t, s, b, gpu, lo, hi): "
                           + str([(tuple(i), got[tuple(i)], lo[tuple(i)], hi[tuple(i)]) for i in bad[:5]]))


@pytest.mark.parametrize("name", list(_POISSON_CASES))
def test_poisson(name):
    S, T, B, off, seed, lam = _POISSON_CASES[name]
    ldb = B + 7
    buf, out = _nan_out(T, S, ldb)
    ops.sample_demand(out, T, S, B, off, seed, 1, _dev(lam), None, True)
    assert _last_kernel() == "sample_poisson_kernel"
    got = _read_back(buf, T, S, ldb, B)
    lo, hi = _poisson_reference(name)
    _in_interval(got, lo, hi, name)
    if name == "past_table":
        assert got.max() > pr.CDF_ENTRIES           # (the continuation past the table is what ran)


def test_poisson_intervals_are_almost_always_one_integer():
    """The interval's width is the only slack of the Poisson cases: the share of draws that have any is at most 1e-4."""
    wide = sum(int((hi > lo).sum()) for lo, hi in map(_poisson_reference, _POISSON_CASES))
    total = sum(lo.size for lo, _ in map(_poisson_reference, _POISSON_CASES))
    print(f"[sampler exact] sample_poisson_kernel: {wide} of {total} draws have an interval wider than one integer ({wide / total:.2e})")
    assert total > 50000 and wide / total <= 1e-4


# the float32 upper tail.  Seed 99, one store, period 0: global scenario indices found on the host by
# philox_reference.scan_poisson_tail (indices 0 .. 1.6e8), with the float32 uniform each one draws.
_TAIL = {
    151_548_650: 1.0,                      # x >= 0xFFFFFF80
    12_493_930: 1.0 - 2.0 ** -24,
    56_632_482: 1.0 - 2.0 ** -24,
    9_272_568: 1.0 - 2.0 ** -23,           # above the last entry of lambda = 5's table (1 - 3 * 2^-24), below 1 - 2^-24
    24_186_642: 1.0 - 2.0 ** -23,
    19_181_280: 1.0 - 3 * 2.0 ** -24,      # equal to that last entry: the last in-range draw
}


@pytest.mark.parametrize("lam", [0.7, 5.0, 12.0, 45.0, 80.0])      # (45 and 80: the continuation past the table saturates too)
@pytest.mark.parametrize("hit", list(_TAIL))
def test_poisson_upper_tail(hit, lam):
    """A uniform at or next to 1.0f must still give a draw inside the accepted interval (for lambda = 5 its upper end is in the
    twenties), whatever the float32 table saturates at.  Before the search stopped where the CDF stops growing, the kernel ran
    its continuation to the cap and wrote 1000 for lambda = 5 at 9,272,568 / 24,186,642 (u = 1 - 2^-23), 12,493,930 / 56,632,482
    (u = 1 - 2^-24) and 151,548,650 (u = 1.0f); at 19,181,280 (u equal to the table's top) it wrote 21, which all of them give
    now.  lambda = 0.7 (8 or 9) and lambda = 12 (32 or 33) were inside their intervals before and are unchanged: those tables end
    at 1.0 and above it."""
    u = pr.u01_f32(pr.poisson_uniforms(99, [hit], 1, 1)[0, 0, 0])
    assert u == np.float32(_TAIL[hit])
    table_last = pr.poisson_table_f32(lam)[-1]
    T, B, off = 1, 8, hit - 3
    buf, out = _nan_out(T, 1, 16)
    ops.sample_demand(out, T, 1, B, off, 99, 1, _dev([lam]), None, True)
    assert _last_kernel() == "sample_poisson_kernel"
    got = _read_back(buf, T, 1, 16, B)
    lo, hi = pr.poisson_interval(99, off + np.arange(B), T, [lam])
    print(f"[sampler exact] tail: scenario {hit} u = {float(u)!r} lambda = {lam} (replica table ends at {float(table_last)!r}): "
          f"gpu {got[0, 0, 3]:.0f}, accepted [{lo[0, 0, 3]}, {hi[0, 0, 3]}]")
    assert lam < hi[0, 0, 3] < lam + 10 * np.sqrt(lam) + 12 and (lam != 5.0 or 20 <= hi[0, 0, 3] <= 29)
    _in_interval(got, lo, hi, f"tail scenario {hit} lambda {lam}")


# ---- rejections ----------------------------------------------------------------------------------------------------------------

def test_bad_arguments_raise_and_launch_nothing():
    T, S, B, ldb = 3, 4, 40, 48
    mean, std = _dev(np.full(S, 5.0)), _dev(np.ones(S))
    L = _dev(np.eye(S)).contiguous()
    buf, out = _nan_out(T, S, ldb)
    marker = torch.full((8,), float("nan"), device=DEV)
    ops.sample_demand_equicorrelated(marker.view(1, 1, 8), 1, 1, 4, 0, 1, mean[:1], std[:1], 0.0, False)   # the last launch on record
    assert _last_kernel() == "sample_one_store_kernel"

    def rejected(call):
        with pytest.raises(NicError):
            call()
        assert _last_kernel() == "sample_one_store_kernel"       # nothing was launched after the marker

    rejected(lambda: ops.sample_demand(out, T, S, B, 0, 1, 2, mean, L, False))                          # kind = 2
    rejected(lambda: ops.sample_demand_equicorrelated(out, T, S, B, 0, 1, mean, std, -0.1, False))
    rejected(lambda: ops.sample_demand_equicorrelated(out, T, S, B, 0, 1, mean, std, 1.1, False))
    rejected(lambda: ops.sample_demand(out, T, S, B, 0, 1, 0, mean, None, False))                       # normal kind, no factor
    rejected(lambda: ops.sample_demand(out, T, S, ldb + 1, 0, 1, 1, mean, None, True))                  # ldb < n_scenarios
    rejected(lambda: ops.sample_demand_equicorrelated(out, T, S, ldb + 1, 0, 1, mean, std, 0.5, False))
    assert np.isnan(_read_back(buf, T, S, ldb, B)).all()
    # T = 65,536 (the grid's y dimension ends at 65,535), on a buffer that could hold it
    bufT, outT = _nan_out(65536, 1, 8)
    rejected(lambda: ops.sample_demand_equicorrelated(outT, 65536, 1, 4, 0, 1, mean[:1], std[:1], 0.0, False))
    rejected(lambda: ops.sample_demand(outT, 65536, 1, 4, 0, 1, 1, mean[:1], None, True))
    assert np.isnan(_read_back(bufT, 65536, 1, 8, 4)).all()
    # more stores than the general-covariance sampler takes
    S97 = 97
    buf97, out97 = _nan_out(1, S97, 8)
    rejected(lambda: ops.sample_demand(out97, 1, S97, 4, 0, 1, 0, _dev(np.ones(S97)), _dev(np.eye(S97)).contiguous(), False))
    assert np.isnan(_read_back(buf97, 1, S97, 8, 4)).all()


# ---- Scenario wiring -----------------------------------------------------------------------------------------------------------

def _scenario(workload, n, k, T, edit=None):
    from neural_inventory_control_amd import workloads
    from neural_inventory_control_amd.data_handling import Scenario
    setting = copy.deepcopy(workloads.get(workload)[0])
    if edit:
        edit(setting)
    obs = defaultdict(lambda: None, setting["observation_params"])
    return Scenario(T, setting["problem_params"], setting["store_params"], setting["warehouse_params"], setting["echelon_params"],
                    n, obs, dict(setting["seeds"]), sampler="hip", device=DEV, scenario_offset=k)


def _scenario_trace(sc, n, T):
    pp, dp, seed = sc._device_sampler_args          # the parameters Scenario ended up with
    S = pp["n_stores"]
    soa = sc.demands_soa
    assert soa.shape[:2] == (T, S) and soa.shape[2] >= n
    torch.cuda.synchronize()
    assert float(soa[:, :, n:].abs().sum()) == 0.0
    assert torch.equal(sc.demands, soa[:, :, :n].permute(2, 1, 0))
    return S, dp, int(seed), soa[:, :, :n].double().cpu().numpy()


def _negative(setting):
    setting["store_params"]["demand"]["correlation"] = -0.05


@pytest.mark.parametrize("workload,edit,kernel", [("cfg3", None, "sample_equicorrelated_kernel<1>"),
                                                  ("cfg3", _negative, "sample_cholesky_kernel<16>")])
def test_scenario_normal_trace_is_the_builders(workload, edit, kernel):
    n, k, T = 64, 5, 6
    sc = _scenario(workload, n, k, T, edit)
    assert _last_kernel() == kernel
    S, dp, seed, got = _scenario_trace(sc, n, T)
    assert S > 1
    mean = np.broadcast_to(np.asarray(dp["mean"], dtype=np.float32), (S,))
    std = np.broadcast_to(np.asarray(dp["std"], dtype=np.float32), (S,))
    rho = float(dp["correlation"])
    if edit is None:
        want, band = pr.equicorrelated(seed, k + np.arange(n), T, mean, std, rho, bool(dp["clip"]))
    else:
        assert rho < 0
        cov = np.asarray(sc._covariance(dp), dtype=np.float64)
        assert cov[0, 1] < 0 and cov.shape == (S, S)
        want, band = pr.general_covariance(seed, k + np.arange(n), T, mean, np.linalg.cholesky(cov).astype(np.float32), bool(dp["clip"]))
    _in_band(kernel, got, want, band, f"Scenario({workload}, offset {k})")


def test_scenario_poisson_trace_is_the_builders():
    n, k, T = 64, 5, 6
    sc = _scenario("cfg1", n, k, T)
    assert _last_kernel() == "sample_poisson_kernel"
    S, dp, seed, got = _scenario_trace(sc, n, T)
    assert dp["distribution"] == "poisson"
    lam = np.broadcast_to(np.asarray(dp["mean"], dtype=np.float32), (S,))
    lo, hi = pr.poisson_interval(seed, k + np.arange(n), T, lam)
    _in_interval(got, lo, hi, f"Scenario(cfg1, offset {k})")


def test_scenario_rejects_a_poisson_mean_beyond_the_samplers_range():
    def too_large(setting):
        setting["store_params"]["demand"]["mean"] = ops.SAMPLER_POISSON_MAX_MEAN + 0.5
    with pytest.raises(ValueError, match="Poisson"):
        _scenario("cfg1", 64, 5, 6, too_large)

    def largest(setting):
        setting["store_params"]["demand"]["mean"] = ops.SAMPLER_POISSON_MAX_MEAN
    sc = _scenario("cfg1", 64, 5, 6, largest)
    assert ops.SAMPLER_POISSON_MAX_MEAN >= 80.0
    S, dp, seed, got = _scenario_trace(sc, 64, 6)
    lo, hi = pr.poisson_interval(seed, 5 + np.arange(64), 6, [ops.SAMPLER_POISSON_MAX_MEAN])
    _in_interval(got, lo, hi, "Scenario(cfg1, largest mean)")
