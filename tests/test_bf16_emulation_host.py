"""The bounds of tests/bf16_emulation.py, judged on the CPU: MEETABLE (a correct FP32-accumulating implementation stays inside
them, whatever its summation order) and with POWER (each way a bf16 GEMM kernel goes subtly wrong leaves them by >= 10x).  This
is what makes a green run of tests/test_gpu_bf16.py mean something; no GPU is needed.

Inputs are the GPU sweep's: weights N(0, 1/K), activations ELU(N(0, 1)) (mixed sign, as the hidden layers see), pre-activation
gradients 1e-3 N(0, 1), all FP32 with full mantissas.  Full mantissas matter for the truncation mutant (values that are already
bf16 would hide it); the mixed signs are the HARD case for it (truncation errors of opposite-sign products cancel), so it is
caught where it is hardest.  The tile mutants drop / double / swap O(1/10) of each sum, orders of magnitude above K * 2^-24."""
import pytest
import torch

import bf16_emulation as emu

SHAPES = [(160, 224), (128, 128)]
NCOLS = 300   # "a few hundred columns"; not a multiple of 32 (a partial last scenario tile)
POWER = 10.0


def _inputs(N, K, n, seed):
    g = torch.Generator().manual_seed(seed)
    W = torch.randn(N, K, generator=g) * K ** -0.5
    X = emu.elu(torch.randn(K, n, generator=g).double()).float()
    bias = torch.randn(N, generator=g) * 0.1
    dY = torch.randn(N, n, generator=g) * 1e-3
    H = emu.elu(torch.randn(K, n, generator=g).double()).float()
    prev = torch.randn(K, n, generator=g) * 1e-3
    return W, X, bias, dY, H, prev


def _rne(t):
    return t.to(torch.bfloat16).float()


def _trunc(t):
    return (t.contiguous().view(torch.int32) & -65536).view(torch.float32)


def _mm_chunked(a, b, chunk):
    """FP32 a @ b with the contraction cut into chunks whose FP32 partial sums are added one after the other (the slab's order)"""
    out = torch.zeros(a.shape[0], b.shape[1])
    for k0 in range(0, a.shape[1], chunk):
        out = out + a[:, k0:k0 + chunk] @ b[k0:k0 + chunk]
    return out


def _elu32(z):
    return torch.where(z > 0, z, torch.expm1(torch.clamp(z, max=0)))


def _fwd(W, X, bias, rnd=_rne, mm=torch.matmul):
    return _elu32(mm(rnd(W), rnd(X)) + bias[:, None])


def _dgrad(W, dY, H, prev, rnd=_rne, mm=torch.matmul):
    return mm(rnd(W.t().contiguous()), rnd(dY)) * torch.where(H > 0, torch.ones_like(H), H + 1) + prev


def _wgrad(dY, X, rnd=_rne, mm=torch.matmul):
    return mm(rnd(dY), rnd(X).t().contiguous()), dY.sum(1)


def _swap_halves(a):
    """columns (k) of `a` with the two 8-element halves of every 16-deep MFMA step exchanged"""
    k = torch.arange(a.shape[1])
    return a[:, k ^ 8]


@pytest.mark.parametrize("N,K", SHAPES)
def test_bounds_are_meetable(N, K):
    W, X, bias, dY, H, prev = _inputs(N, K, NCOLS, 1)
    worst = {}
    for name, mm in (("one sum", torch.matmul), ("chunks of 32", lambda a, b: _mm_chunked(a, b, 32)),
                     ("chunks of 96", lambda a, b: _mm_chunked(a, b, 96))):
        ref, tol = emu.forward(W, X, bias)
        worst[f"forward, {name}"] = emu.worst(_fwd(W, X, bias, mm=mm), ref, tol)
        ref, tol = emu.forward(W, X, None, act_elu=False)
        worst[f"forward (identity), {name}"] = emu.worst(mm(_rne(W), _rne(X)), ref, tol)
        ref, tol = emu.dgrad(W.t(), dY, H, prev)
        worst[f"dgrad, {name}"] = emu.worst(_dgrad(W, dY, H, prev, mm=mm), ref, tol)
        ref, tol = emu.dgrad(W.t(), dY)
        worst[f"dgrad (no activation), {name}"] = emu.worst(mm(_rne(W.t().contiguous()), _rne(dY)), ref, tol)
        ref, tol, ref_b, tol_b = emu.wgrad(dY, X)
        gw, gb = _wgrad(dY, X, mm=mm)
        worst[f"wgrad, {name}"] = emu.worst(gw, ref, tol)
        worst[f"bias gradient, {name}"] = emu.worst(gb, ref_b, tol_b)
    # the weight gradient into a slab that is not zero to begin with, in slots of 64 scenarios, deltas summed in float64
    base = torch.full((5, N, K + 1), 2.0 ** -10)
    slab = base.clone()
    for s in range(5):
        sl = slice(64 * s, 64 * (s + 1))
        gw, gb = _wgrad(dY[:, sl], X[:, sl])
        slab[s, :, :K] += gw
        slab[s, :, K] += gb
    delta = (slab.double() - base.double()).sum(0)
    ref, tol, ref_b, tol_b = emu.wgrad(dY, X, base_w=base[:, :, :K].abs().amax(0), base_b=base[:, :, K].abs().amax(0))
    worst["wgrad into a pre-filled slab"] = max(emu.worst(delta[:, :K], ref, tol), emu.worst(delta[:, K], ref_b, tol_b))
    # two periods through wgrad_periods
    dYh, Xh = torch.stack([dY, dY.flip(1)]), torch.stack([X, X.flip(0)])
    ref, tol, ref_b, tol_b = emu.wgrad_periods(dYh, Xh)
    gw = sum(_wgrad(dYh[t], Xh[t])[0] for t in range(2))
    worst["wgrad over periods"] = emu.worst(gw, ref, tol)
    print({k: round(v, 4) for k, v in worst.items()})
    assert max(worst.values()) <= 1.0, worst
    assert min(worst.values()) > 0.0, worst   # (FP32 accumulation does differ from the float64 reference: the ratio is a real one)


@pytest.mark.parametrize("N,K", SHAPES)
def test_bounds_catch_every_mutant(N, K):
    W, X, bias, dY, H, prev = _inputs(N, K, NCOLS, 2)
    f_ref, f_tol = emu.forward(W, X, bias)
    d_ref, d_tol = emu.dgrad(W.t(), dY, H, prev)
    w_ref, w_tol, b_ref, b_tol = emu.wgrad(dY, X)
    a, b = _rne(W), _rne(X)
    caught = {}

    # 1. truncation instead of round to nearest even, in every entry point
    caught["truncation, forward"] = emu.worst(_fwd(W, X, bias, rnd=_trunc), f_ref, f_tol)
    caught["truncation, dgrad"] = emu.worst(_dgrad(W, dY, H, prev, rnd=_trunc), d_ref, d_tol)
    caught["truncation, wgrad"] = emu.worst(_wgrad(dY, X, rnd=_trunc)[0], w_ref, w_tol)

    # 2. the two 8-element k halves of a 16-deep MFMA step swapped for ONE operand (a wrong fragment lane map)
    caught["k halves swapped in A, forward"] = emu.worst(_elu32(_swap_halves(a) @ b + bias[:, None]), f_ref, f_tol)
    caught["k halves swapped in B, forward"] = emu.worst(_elu32(a @ _swap_halves(b.t()).t() + bias[:, None]), f_ref, f_tol)
    caught["scenario halves swapped in dY, wgrad"] = emu.worst(_swap_halves(_rne(dY)[:, :288]) @ _rne(X)[:, :288].t()
                                                               + _rne(dY)[:, 288:] @ _rne(X)[:, 288:].t(), w_ref, w_tol)

    # 3. one 32-deep k tile dropped (the last one: a double buffer that is not drained; and one in the middle)
    for name, k0 in (("last", K - 32), ("second", 32)):
        keep = torch.ones(K, dtype=torch.bool)
        keep[k0:k0 + 32] = False
        caught[f"{name} k tile dropped, forward"] = emu.worst(_elu32(a[:, keep] @ b[keep] + bias[:, None]), f_ref, f_tol)
        at, dy = _rne(W.t().contiguous()), _rne(dY)
        keep_n = torch.ones(N, dtype=torch.bool)
        keep_n[(k0 % N):(k0 % N) + 32] = False
        got = (at[:, keep_n] @ dy[keep_n]) * torch.where(H > 0, torch.ones_like(H), H + 1) + prev
        caught[f"{name} k tile dropped, dgrad"] = emu.worst(got, d_ref, d_tol)

    # 4. one 32-scenario tile counted twice in the weight gradient (a flush segment restarted one tile early)
    gw, gb = _wgrad(dY, X)
    gw2, gb2 = _wgrad(dY[:, 64:96], X[:, 64:96])
    caught["scenario tile doubled, wgrad"] = emu.worst(gw + gw2, w_ref, w_tol)
    caught["scenario tile doubled, bias gradient"] = emu.worst(gb + gb2, b_ref, b_tol)
    caught["scenario tile dropped, wgrad"] = emu.worst(gw - gw2, w_ref, w_tol)

    # 5. rows / columns at or beyond the matrix read as data instead of zero.  The contraction lengths are multiples of 32, so
    # such a row only ever reaches an OUTPUT row or column at or beyond M: what goes wrong is a write there.  In the weight
    # gradient that is slab column K - the bias gradient - and the columns behind it: X's row K (whatever follows X in memory)
    # lands on them.  The forward's rows beyond M land in the rows that follow Y: the sweep keeps guard rows there.
    lds = K + 4
    Xext = torch.cat([X, torch.randn(4, NCOLS, generator=torch.Generator().manual_seed(3))])   # rows K.. : the next tensor
    slab = torch.zeros(N, lds)
    slab[:, :K], slab[:, K] = gw, gb
    mutant = slab.clone()
    mutant[:, K:] += _rne(dY) @ _rne(Xext[K:]).t()
    assert emu.worst(slab[:, K], b_ref, b_tol) <= 1.0 and not slab[:, K + 1:].any()
    caught["X rows beyond K counted, bias column of the slab"] = emu.worst(mutant[:, K], b_ref, b_tol)
    assert mutant[:, K + 1:].any()   # ... and the columns beyond K + 1 are written (the sweep requires them untouched)

    # 6. padding columns counted in the weight gradient (garbage beyond n_scenarios, as the sweep puts there)
    pad = torch.randn(max(N, K), 4, generator=torch.Generator().manual_seed(4))
    gwp, gbp = _wgrad(torch.cat([dY, pad[:N] * 1e-3], 1), torch.cat([X, pad[:K]], 1))
    caught["padding columns counted, wgrad"] = emu.worst(gwp, w_ref, w_tol)
    caught["padding columns counted, bias gradient"] = emu.worst(gbp, b_ref, b_tol)
    gw1, gb1 = _wgrad(torch.cat([dY, pad[:N, :1] * 1e-3], 1), torch.cat([X, pad[:K, :1]], 1))
    caught["ONE padding column counted, wgrad"] = emu.worst(gw1, w_ref, w_tol)

    print({k: round(v, 1) for k, v in caught.items()})
    missed = {k: v for k, v in caught.items() if not v >= POWER}
    assert not missed, missed


def test_long_contractions_need_the_tile_scan():
    """12,288 terms (a weight gradient over 3 periods of 4,096 scenarios: the shortest that crosses a flush segment has more than
    8,192): the dense bound does NOT show one lost 32-scenario tile any more - the tile scan of bf16_emulation does, in the pass
    that holds the tile, while the correct FP32 sum stays inside the bound in every pass."""
    N, K, T, n = 128, 128, 3, 4096
    g = torch.Generator().manual_seed(5)
    dYh, Xh = torch.randn(T, N, n, generator=g) * 1e-3, torch.randn(T, K, n, generator=g)

    def fp32_sum(dY, X, lose=None):
        out = torch.zeros(N, K)
        for t in range(T):
            for b0 in range(0, n, 2048):   # (slab order: chunks of 2,048 scenarios, period after period)
                out = out + _rne(dY[t, :, b0:b0 + 2048]) @ _rne(X[t, :, b0:b0 + 2048]).t()
        if lose is not None:
            t, b0 = lose
            out = out - _rne(dY[t, :, b0:b0 + 32]) @ _rne(X[t, :, b0:b0 + 32]).t()
        return out

    lost = (1, 2048)   # the first tile of a chunk of the second period
    ref, tol, _, _ = emu.wgrad_periods(dYh, Xh)
    assert emu.worst(fp32_sum(dYh, Xh), ref, tol) <= 1.0
    dense = emu.worst(fp32_sum(dYh, Xh, lost), ref, tol)
    assert dense < POWER, dense   # (why the scan exists; if this ever fails the dense check has become strong enough)
    m = emu.tile_scan_stride(T * n)
    assert m == 8
    dYa, Xa = dYh.abs(), Xh.abs()
    lost_tile = lost[0] * (n // 32) + lost[1] // 32
    ok, caught = 0.0, 0.0
    for r in range(m):
        dYm = dYa * emu.tile_mask(T, n, n, m, r, "cpu")[:, None, :]
        ref, tol, _, _ = emu.wgrad_periods(dYm, Xa)
        ok = max(ok, emu.worst(fp32_sum(dYm, Xa), ref, tol))
        if lost_tile % m == r:
            caught = emu.worst(fp32_sum(dYm, Xa, lost), ref, tol)
    print({"dense, tile lost": round(dense, 2), "scan, correct": round(ok, 4), "scan, tile lost": round(caught, 1)})
    assert ok <= 1.0 and caught >= POWER, (ok, caught)
