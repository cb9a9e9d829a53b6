"""Host reference of csrc/sampler.hip, draw for draw (numpy + scipy only; importable without a GPU).

The sampler's contract is that every number is a pure function of (seed, GLOBAL scenario index, period, variate).  This module
computes that function on the host: Philox4x32-10 in uint64 arithmetic (constants from the Random123 specification, not from
the kernel), the kernel's 32 bits -> float32 uniform conversion bit for bit, and everything after it in float64.  One builder
per kernel returns the float64 demands [T][S][n] of the given global scenario indices and, with them, the band inside which
the float32 kernel has to land (the Poisson builder returns an interval of accepted integers instead).

Bands.  Per standard normal z = r * cos|sin(2 pi u_y), r = sqrt(-2 ln u_x):
    tol_z = 4e-6 * (1 + r) + 2^-22 / r
4e-6 is the kernel header's accuracy claim ("~1e-6 on a unit-variance variate") with the x4 margin `_close` of
test_gpu_kernels.py uses, times (1 + r) because a sin / cos error scales with the radius; the 1 / r term carries an absolute
log2 error of a few float32 steps near u -> 1, where dr = 0.69 eps / r.  Per demand: the tol_z of its normals pushed through the
linear map with absolute coefficients, plus 4e-6 * (|mean| + sum |coef z|) + 1e-6 for the float32 arithmetic.
"""
import numpy as np

_U = np.uint64
MASK32 = _U(0xFFFFFFFF)
# Random123 philox4x32: multipliers and Weyl key increments
PHILOX_M0, PHILOX_M1 = _U(0xD2511F53), _U(0xCD9E8D57)
PHILOX_W0, PHILOX_W1 = _U(0x9E3779B9), _U(0xBB67AE85)
_S32 = _U(32)

K_COMMON = 0xFFFFFFFF   # fourth counter word of the equicorrelated sampler's common-factor blocks
K_OWN = 0xFFFFFFFE      # ... of the one-store sampler's blocks
CDF_ENTRIES = 64        # entries of the Poisson kernel's per-store float32 CDF table

TWO_M32_F32 = np.float32(2.3283064365386963e-10)

# Poisson: the kernel inverts a float32 CDF (a 64-entry table built by the recurrence p *= lam / (k + 1), F += p, continued past
# the table for large means), the reference the exact float64 one.  A draw is accepted when it is the quantile of some
# u' within DELTA of the draw's uniform.  DELTA starts at 2^-20 and has to be at least 4 x the largest
# |float32 table - float64 CDF| of a numpy float32 replica of the kernel's recurrence (poisson_table_error below, against scipy's
# float64 CDF) over lam in {0.05, 0.7, 5, 12, 30, 45, 80}.  Measured: 3.144e-7 (5.3 float32 steps of 2^-24, at lam = 12, whose
# table overshoots to 1.0000002; 0.05: 6.0e-8, 0.7: 3.0e-8, 5: 1.8e-7, 30: 8.7e-8, 45: 2.4e-7, 80: 5.5e-9 inside the table).
# 4 x 3.144e-7 = 1.258e-6 > 2^-20, so DELTA is raised to exactly that and no further.  (The continuation past the table, carried
# until F stops growing, strays further at lam = 80: 5.9e-7, still inside DELTA; poisson_table_error(continuation=True).)
POISSON_TABLE_ERROR_MEASURED = 3.144e-7
POISSON_DELTA = max(2.0 ** -20, 4 * POISSON_TABLE_ERROR_MEASURED)   # (test_philox_reference_host.py re-measures and asserts this)
POISSON_U_MAX = 1.0 - 2.0 ** -33        # the largest u64 = (x + 0.5) 2^-32


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32 with 10 rounds.  Counter and key words are integers or integer arrays below 2^32 (broadcast against each other);
    returns the four output words as uint64 arrays holding values below 2^32."""
    c0, c1, c2, c3 = np.broadcast_arrays(*[np.asarray(c, dtype=np.uint64) for c in (c0, c1, c2, c3)])
    k0, k1 = np.asarray(k0, dtype=np.uint64), np.asarray(k1, dtype=np.uint64)
    for _ in range(10):
        p0, p1 = PHILOX_M0 * c0, PHILOX_M1 * c2       # 32 x 32 -> 64 bits: exact in uint64
        c0, c1, c2, c3 = (p1 >> _S32) ^ c1 ^ k0, p1 & MASK32, (p0 >> _S32) ^ c3 ^ k1, p0 & MASK32
        k0, k1 = (k0 + PHILOX_W0) & MASK32, (k1 + PHILOX_W1) & MASK32
    return c0, c1, c2, c3


def u01_f32(x):
    """The kernel's u01, bit for bit: x -> float32 (round to nearest), + 0.5f, * 2^-32, every step in float32 (all three are
    IEEE-exact operations, so both sides agree by construction).  1.0 exactly for x >= 0xFFFFFF80."""
    xf = np.asarray(x, dtype=np.uint64).astype(np.float64).astype(np.float32)   # (exact, then ONE rounding)
    return (xf + np.float32(0.5)) * TWO_M32_F32


def u01_f64(x):
    """(x + 0.5) 2^-32 in float64: exact, inside (0, 1)."""
    return (np.asarray(x, dtype=np.uint64).astype(np.float64) + 0.5) * 2.0 ** -32


def _keys(seed):
    seed = int(seed)
    assert 0 <= seed < 2 ** 64
    return seed & 0xFFFFFFFF, seed >> 32


def _scen(scenarios):
    g = np.asarray(scenarios, dtype=np.uint64).reshape(-1)
    return g & MASK32, g >> _S32


def block_words(seed, scenarios, c2, c3):
    """Words [4, ...] of the blocks (scenario_lo, scenario_hi, c2, c3); c2 / c3 broadcast against scenarios [n]."""
    lo, hi = _scen(scenarios)
    k0, k1 = _keys(seed)
    return np.stack(philox4x32_10(lo, hi, c2, c3, k0, k1))


def normals_of_block(words):
    """Four standard normals of a block in float64 from the kernel's float32 uniforms (two Box-Muller pairs: (x, y) and (z, w)).
    words [4, ...] -> (z [4, ...], r [4, ...]); r is the radius each normal was made with."""
    u = u01_f32(words).astype(np.float64)
    r0, r1 = np.sqrt(-2.0 * np.log(u[0])), np.sqrt(-2.0 * np.log(u[2]))
    a0, a1 = 2.0 * np.pi * u[1], 2.0 * np.pi * u[3]
    z = np.stack([r0 * np.cos(a0), r0 * np.sin(a0), r1 * np.cos(a1), r1 * np.sin(a1)])
    return z, np.stack([r0, r0, r1, r1])


def tol_z(r):
    with np.errstate(divide="ignore"):
        return 4e-6 * (1.0 + r) + 2.0 ** -22 / r


def _own_normals(seed, scenarios, T, S):
    """z, r [T][S][n]: variate s of period t is word s % 4 of block (lo, hi, t, s / 4)."""
    nb = (S + 3) // 4
    t = np.arange(T, dtype=np.uint64)[:, None, None]
    blk = np.arange(nb, dtype=np.uint64)[None, :, None]
    z, r = normals_of_block(block_words(seed, scenarios, t, blk))        # [4][T][nb][n]
    n = z.shape[-1]
    pick = lambda a: np.transpose(a, (1, 2, 0, 3)).reshape(T, nb * 4, n)[:, :S]   # noqa: E731
    return pick(z), pick(r)


def _per_period_normals(seed, scenarios, T, tag):
    """z, r [T][n]: period t takes word t & 3 of block (lo, hi, t >> 2, tag)."""
    t = np.arange(T)
    z, r = normals_of_block(block_words(seed, scenarios, (t >> 2).astype(np.uint64)[:, None], tag))   # [4][T][n]
    return z[t & 3, t], r[t & 3, t]


def _finish(d, band, clip):
    return (np.maximum(d, 0.0) if clip else d), band      # (clipping is 1-Lipschitz: the band stands)


def _f32_params(*arrays):
    """The parameters as the kernel sees them: float32 values, carried in float64."""
    return [np.asarray(a, dtype=np.float32).astype(np.float64).reshape(-1) for a in arrays]


def equicorrelated(seed, scenarios, T, mean, std, rho, clip):
    """sample_equicorrelated_kernel<PER>: d = mean + std (sqrt(rho) z_common + sqrt(1 - rho) z_s).  -> (d, band) [T][S][n]"""
    mean, std = _f32_params(mean, std)
    S = mean.size
    rho = float(np.float32(rho))
    a_c, a_o = np.sqrt(rho), np.sqrt(1.0 - rho)
    zc, rc = _per_period_normals(seed, scenarios, T, K_COMMON)
    zs, rs = _own_normals(seed, scenarios, T, S)
    zc, rc = zc[:, None, :], rc[:, None, :]
    m, s = mean[None, :, None], std[None, :, None]
    d = m + s * (a_c * zc + a_o * zs)
    band = s * (a_c * tol_z(rc) + a_o * tol_z(rs)) + 4e-6 * (np.abs(m) + s * (a_c * np.abs(zc) + a_o * np.abs(zs))) + 1e-6
    return _finish(d, band, clip)


def one_store(seed, scenarios, T, mean, std, clip):
    """sample_one_store_kernel: d = mean + std z, z = word t & 3 of block (lo, hi, t >> 2, K_OWN).  -> (d, band) [T][1][n]"""
    mean, std = _f32_params(mean, std)
    assert mean.size == 1 and std.size == 1
    z, r = _per_period_normals(seed, scenarios, T, K_OWN)
    d = mean[0] + std[0] * z
    band = std[0] * tol_z(r) + 4e-6 * (abs(mean[0]) + std[0] * np.abs(z)) + 1e-6
    d, band = _finish(d, band, clip)
    return d[:, None, :], band[:, None, :]


def general_covariance(seed, scenarios, T, mean, chol, clip):
    """sample_cholesky_kernel<SMAX>: d_s = mean_s + sum_{j <= s} L_sj z_j (the lower triangle only).  -> (d, band) [T][S][n]"""
    mean, = _f32_params(mean)
    S = mean.size
    L = np.tril(np.asarray(chol, dtype=np.float32).astype(np.float64).reshape(S, S))
    z, r = _own_normals(seed, scenarios, T, S)
    # (summed column by column in a fixed order, so that a scenario's value does not depend on which others are evaluated with it)
    apply = lambda M, v: sum(M[None, :, j, None] * v[:, None, j, :] for j in range(S))   # noqa: E731
    d = mean[None, :, None] + apply(L, z)
    band = apply(np.abs(L), tol_z(r)) + 4e-6 * (np.abs(mean)[None, :, None] + apply(np.abs(L), np.abs(z))) + 1e-6
    return _finish(d, band, clip)


def poisson_uniforms(seed, scenarios, T, S):
    """The 32 random bits behind every Poisson draw, [T][S][n] (uint64): word s % 4 of block (lo, hi, t, s / 4)."""
    nb = (S + 3) // 4
    t = np.arange(T, dtype=np.uint64)[:, None, None]
    blk = np.arange(nb, dtype=np.uint64)[None, :, None]
    w = block_words(seed, scenarios, t, blk)
    return np.transpose(w, (1, 2, 0, 3)).reshape(T, nb * 4, w.shape[-1])[:, :S]


def poisson_quantile(q, lam):
    """Exact float64 Poisson quantile: the smallest k with P(X <= k) >= q (0 for q = 0)."""
    from scipy.stats import poisson
    return np.maximum(poisson.ppf(q, lam), 0.0).astype(np.int64)


def poisson_interval(seed, scenarios, T, lam, delta=POISSON_DELTA):
    """sample_poisson_kernel: the accepted integers [lo, hi] of every draw, [T][S][n] each:
    [Q(max(u64 - delta, 0)), Q(min(u64 + delta, 1 - 2^-33))], Q the exact quantile, u64 = (x + 0.5) 2^-32."""
    lam, = _f32_params(lam)
    u = u01_f64(poisson_uniforms(seed, scenarios, T, lam.size))
    lam = np.broadcast_to(lam[None, :, None], u.shape)
    return (poisson_quantile(np.maximum(u - delta, 0.0), lam), poisson_quantile(np.minimum(u + delta, POISSON_U_MAX), lam))


# ---- the kernel's float32 CDF, replicated (for measuring DELTA and for finding tail scenarios; never a reference) --------------

def poisson_table_f32(lam, entries=CDF_ENTRIES):
    """numpy float32 replica of the kernel's recurrence: F[k] = P(X <= k), k < entries.  (The device's expf may differ from
    numpy's by a float32 step, so this is a replica of the arithmetic, not of the bits.)"""
    lam = np.float32(lam)
    p = np.exp(-lam, dtype=np.float32)
    F = p
    out = np.empty(entries, dtype=np.float32)
    for k in range(entries):
        out[k] = F
        p = p * (lam / np.float32(k + 1))
        F = F + p
    return out


POISSON_LAMBDAS = (0.05, 0.7, 5.0, 12.0, 30.0, 45.0, 80.0)


def poisson_table_error(lams=POISSON_LAMBDAS, continuation=False):
    """Largest |float32 table - float64 CDF| over the given means; with `continuation` the recurrence is carried past the table
    as the kernel does (p = c[63] - c[62], p *= lam / k, F += p) until F stops growing."""
    from scipy.stats import poisson
    worst = 0.0
    for lam in lams:
        c = poisson_table_f32(lam)
        vals = list(c)
        lam32, F, p, k = np.float32(lam), c[-1], c[-1] - c[-2], CDF_ENTRIES - 1
        while continuation and k < 1000:
            k += 1
            p = p * (lam32 / np.float32(k))
            if F + p == F:
                break
            F = F + p
            vals.append(F)
        vals = np.asarray(vals, dtype=np.float64)
        worst = max(worst, float(np.abs(vals - poisson.cdf(np.arange(vals.size), float(lam32))).max()))
    return worst


def scan_poisson_tail(seed, first, count, chunk=1 << 22):
    """Global scenario indices in [first, first + count) whose (one store, period 0) Poisson uniform lies in the float32 upper
    tail: {index: float32 u} for every u >= 1 - 2^-22.  Block (lo, hi, 0, 0), word 0."""
    hits = {}
    k0, k1 = _keys(seed)
    for lo in range(first, first + count, chunk):
        g = np.arange(lo, min(lo + chunk, first + count), dtype=np.uint64)
        x = philox4x32_10(g & MASK32, g >> _S32, 0, 0, k0, k1)[0]
        for i in np.nonzero(x >= _U(0xFFFFFC00))[0]:
            u = float(u01_f32(x[i]))
            if u >= 1.0 - 2.0 ** -22:
                hits[int(g[i])] = u
    return hits
