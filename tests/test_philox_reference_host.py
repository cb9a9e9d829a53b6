"""tests/philox_reference.py checked on its own, without a GPU: Philox known answers, the uniform conversion's edge values, the
builders' distributions against their parameters (every statistic within 5 standard errors, derived from the sample size) and
their independence of the evaluation order.  tests/test_gpu_sampler_exact.py then holds csrc/sampler.hip to these builders."""
import numpy as np
import pytest

import philox_reference as pr

SEED = 20240607
T, N = 8, 25000          # 2 * 10^5 draws per store
SE = 5.0


@pytest.mark.parametrize("ctr,key,want", [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox4x32_10_known_answers(ctr, key, want):
    """The Random123 known-answer vectors of philox4x32-10."""
    assert " ".join("%08x" % int(w) for w in pr.philox4x32_10(*ctr, *key)) == want
    # vectorised: the same block inside an array of counters
    c0 = np.array([5, ctr[0], 7], dtype=np.uint64)
    got = pr.philox4x32_10(c0, ctr[1], ctr[2], ctr[3], *key)
    assert " ".join("%08x" % int(w[1]) for w in got) == want
    assert all(int(w.max()) < 2 ** 32 for w in got)


def test_u01_replica_edges():
    assert pr.u01_f32(0xFFFFFF80) == np.float32(1.0) and pr.u01_f32(0xFFFFFFFF) == np.float32(1.0)
    assert pr.u01_f32(0) == np.float32(2.0 ** -33)
    assert pr.u01_f32(0xFFFFFF7F) == np.float32(1.0 - 2.0 ** -24)
    assert pr.u01_f32(0).dtype == np.float32
    x = np.array([0, 1, 0x7FFFFFFF, 0xFFFFFFFF], dtype=np.uint64)
    u = pr.u01_f64(x)
    assert u.min() == 2.0 ** -33 and u.max() == pr.POISSON_U_MAX < 1.0
    # the float32 conversion rounds the exact value once: never further than half a float32 step of 1.0 from it
    big = np.arange(0xFFFFF000, 0x100000000, 37, dtype=np.uint64)
    assert np.abs(pr.u01_f32(big).astype(np.float64) - pr.u01_f64(big)).max() <= 2.0 ** -25


def _moments(x, mean, cov):
    """x [S][n] against N(mean, cov): every statistic within SE standard errors."""
    n = x.shape[1]
    sd = np.sqrt(np.diag(cov))
    assert (np.abs(x.mean(axis=1) - mean) <= SE * sd / np.sqrt(n)).all()
    got = np.atleast_2d(np.cov(x))
    se_cov = np.sqrt((np.outer(np.diag(cov), np.diag(cov)) + cov ** 2) / n)   # Var(s_ij) = (c_ii c_jj + c_ij^2) / n
    assert (np.abs(got - cov) <= SE * se_cov).all(), np.abs(got - cov) / se_cov
    z = (x - x.mean(axis=1, keepdims=True)) / x.std(axis=1, keepdims=True)
    assert (np.abs((z ** 3).mean(axis=1)) <= SE * np.sqrt(6.0 / n)).all()
    assert (np.abs((z ** 4).mean(axis=1) - 3.0) <= SE * np.sqrt(24.0 / n)).all()


def _flat(d):
    return np.transpose(d, (1, 0, 2)).reshape(d.shape[1], -1)


@pytest.mark.parametrize("rho", [0.0, 0.3, 1.0])
def test_equicorrelated_builder_has_its_covariance(rho):
    mean = np.array([5.0, 3.0, 7.0, 4.0, 6.0], dtype=np.float32)
    std = np.array([1.5, 1.0, 2.0, 0.8, 1.2], dtype=np.float32)
    d, band = pr.equicorrelated(SEED, np.arange(N), T, mean, std, rho, False)
    assert d.shape == band.shape == (T, 5, N) and d.dtype == np.float64
    r32 = float(np.float32(rho))
    cov = r32 * np.outer(std, std).astype(np.float64)
    cov[np.diag_indices(5)] = std.astype(np.float64) ** 2
    _moments(_flat(d), mean.astype(np.float64), cov)
    assert band.min() > 0 and np.median(band) < 1e-4
    # periods are independent: the common factor of neighbouring periods comes from one block, as different words
    a, b = d[0, 0], d[1, 0]
    assert abs(np.corrcoef(a, b)[0, 1]) <= SE / np.sqrt(N)
    clipped, _ = pr.equicorrelated(SEED, np.arange(100), T, mean * 0, std, rho, True)
    free, _ = pr.equicorrelated(SEED, np.arange(100), T, mean * 0, std, rho, False)
    assert clipped.min() == 0.0 and np.array_equal(clipped, np.maximum(free, 0.0))


def test_one_store_builder_is_normal():
    d, band = pr.one_store(SEED, np.arange(N), T, [5.0], [1.6], False)
    assert d.shape == band.shape == (T, 1, N)
    _moments(_flat(d), np.array([5.0]), np.array([[np.float64(np.float32(1.6)) ** 2]]))
    # neighbouring periods are words of one block, neighbouring scenarios neighbouring blocks
    assert abs(np.corrcoef(d[0, 0], d[1, 0])[0, 1]) <= SE / np.sqrt(N)
    assert abs(np.corrcoef(d[:, 0, :-1].ravel(), d[:, 0, 1:].ravel())[0, 1]) <= SE / np.sqrt(T * (N - 1))


def test_general_covariance_builder_has_its_covariance():
    S = 6
    rng = np.random.default_rng(3)
    A = rng.standard_normal((S, S)) * 0.6
    cov = A @ A.T + np.eye(S)
    assert (cov < 0).any()
    L = np.linalg.cholesky(cov).astype(np.float32)
    mean = np.linspace(3.0, 9.0, S).astype(np.float32)
    # the upper triangle of what is passed is not part of the factor
    d, band = pr.general_covariance(SEED, np.arange(N), T, mean, L + np.triu(np.full((S, S), 9.0, np.float32), 1), False)
    assert d.shape == band.shape == (T, S, N)
    L64 = L.astype(np.float64)
    _moments(_flat(d), mean.astype(np.float64), L64 @ L64.T)


def test_poisson_builder_is_poisson_and_almost_always_decided():
    lam = np.array([0.05, 0.7, 5.0, 12.0, 30.0], dtype=np.float32)
    lo, hi = pr.poisson_interval(SEED, np.arange(N), T, lam)
    assert lo.shape == hi.shape == (T, 5, N) and (lo <= hi).all() and lo.min() >= 0
    share = float((hi > lo).mean())
    print("ambiguous share", share, "expected about", 2 * pr.POISSON_DELTA * np.mean([4, 7, 19, 31, 47]))
    assert share <= 1e-4
    mid = _flat((lo + hi) / 2.0)
    n = mid.shape[1]
    lam64 = lam.astype(np.float64)
    assert (np.abs(mid.mean(axis=1) - lam64) <= SE * np.sqrt(lam64 / n)).all()
    # Var(s^2) = (mu4 - sigma^4) / n, mu4 = lam + 3 lam^2 for a Poisson variate
    assert (np.abs(mid.var(axis=1, ddof=1) - lam64) <= SE * np.sqrt((lam64 + 2 * lam64 ** 2) / n)).all()
    assert (np.abs((mid == 0).mean(axis=1) - np.exp(-lam64)) <= SE * np.sqrt(np.exp(-lam64) * (1 - np.exp(-lam64)) / n) + 1e-4).all()


def test_poisson_delta_covers_the_float32_table():
    """DELTA is max(2^-20, 4 x the measured error of the float32 table replica) and not more."""
    measured = pr.poisson_table_error()
    print("float32 table replica against the float64 CDF:", measured, "=", measured / 2.0 ** -24, "steps of 2^-24;",
          "with the continuation:", pr.poisson_table_error(continuation=True))
    assert measured <= pr.POISSON_TABLE_ERROR_MEASURED <= 1.001 * measured
    assert pr.POISSON_DELTA == max(2.0 ** -20, 4 * pr.POISSON_TABLE_ERROR_MEASURED) >= 4 * measured
    assert pr.poisson_table_error(continuation=True) < pr.POISSON_DELTA
    # the replica's last entries, as the tail cases of the GPU test assume them
    assert pr.poisson_table_f32(5.0)[-1] == np.float32(1.0 - 3 * 2.0 ** -24)
    assert pr.poisson_table_f32(0.7)[-1] == np.float32(1.0)
    assert pr.poisson_table_f32(12.0)[-1] > np.float32(1.0)


def test_poisson_quantile_is_the_smallest_k_reaching_q():
    from scipy.stats import poisson
    q = np.array([0.0, 1e-12, 0.5, 1.0 - 1e-6, pr.POISSON_U_MAX])
    for lam in (0.05, 5.0, 80.0):
        k = pr.poisson_quantile(q, lam)
        assert (poisson.cdf(k, lam) >= q).all() and (k >= 0).all()
        assert ((k == 0) | (poisson.cdf(k - 1, lam) < q)).all()
    assert 20 <= pr.poisson_quantile(pr.POISSON_U_MAX, 5.0) <= 29


def test_builders_do_not_depend_on_evaluation_order():
    """Scenarios [a, b) in one call equal the same scenarios one by one (and in another order): a pure function of the index."""
    a, b = 2 ** 32 - 3, 2 ** 32 + 4           # straddles the carry into the second counter word
    scen = np.arange(a, b, dtype=np.uint64)
    mean, std = np.array([1.0, 2.0, 0.5, 3.0, 2.5], np.float32), np.array([1.0, 0.5, 2.0, 1.5, 0.7], np.float32)
    L = np.linalg.cholesky(np.eye(5) + 0.3).astype(np.float32)
    lam = np.array([0.7, 5.0, 30.0, 45.0, 12.0], np.float32)
    calls = {
        "equicorrelated": lambda s: pr.equicorrelated(SEED, s, 6, mean, std, 0.3, True),
        "one_store": lambda s: pr.one_store(SEED, s, 6, mean[:1], std[:1], True),
        "general": lambda s: pr.general_covariance(SEED, s, 6, mean, L, False),
        "poisson": lambda s: pr.poisson_interval(SEED, s, 6, lam),
    }
    for name, f in calls.items():
        whole = f(scen)
        for part in (0, 1):
            single = np.concatenate([f(scen[i:i + 1])[part] for i in range(scen.size)], axis=2)
            assert np.array_equal(whole[part], single), name
            assert np.array_equal(f(scen[::-1])[part], whole[part][:, :, ::-1]), name
    # and the two counter words are both in use: scenario 2^32 is not scenario 0
    assert not np.array_equal(calls["one_store"](np.array([0]))[0], calls["one_store"](np.array([2 ** 32]))[0])
    # the high key word is in use
    assert not np.array_equal(pr.one_store(5, scen, 6, [1.0], [1.0], False)[0], pr.one_store(5 + 2 ** 32, scen, 6, [1.0], [1.0], False)[0])


def test_tail_scan_finds_the_recorded_scenarios():
    """The two scenarios the sampler's tail cases start from (seed 99, one store, period 0)."""
    hits = pr.scan_poisson_tail(99, 9_272_000, 1000)
    assert hits == {9_272_568: float(np.float32(1.0 - 2.0 ** -23))}
    x = pr.poisson_uniforms(99, [9_272_568, 12_493_930], 1, 1)[0, 0]
    assert int(x[0]) == 4294966887
    assert list(pr.u01_f32(x)) == [np.float32(1.0 - 2.0 ** -23), np.float32(1.0 - 2.0 ** -24)]
