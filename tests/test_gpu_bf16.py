"""Opt-in bf16 GEMMs of the wide hidden layers (csrc/linear_bf16.hip, FusedRollout.gemm_precision = "bf16") on the GPU.

The kernels are checked against an EXACT emulation: operands rounded to bf16 by torch, contracted in fp64.  The only difference
the kernels may show is FP32 accumulation: |C - C_ref| <= n * 2^-24 * sum |a b| per element (n = terms of the contraction), plus
the rounding of the FP32 bias add and the ELU / ELU' epilogue.  A wrong lane map or a truncating conversion misses that by orders
of magnitude.  The engine in bf16 mode is compared with the FP32 engine (the parity-checked default) on the workloads' shapes."""
import copy
from collections import defaultdict

import pytest
import torch

import bf16_emulation as emu
from neural_inventory_control_amd import _lib, main_run, ops, workloads
from neural_inventory_control_amd.data_handling import Scenario
from neural_inventory_control_amd.loss_functions import PolicyLoss
from neural_inventory_control_amd.neural_networks import NeuralNetworkCreator
from neural_inventory_control_amd.rollout import FusedRollout

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = emu.U
_bf, _elu, _within = emu.bf, emu.elu, emu.within


def _rand(*shape, scale=1.0, gen=None):
    return (torch.randn(*shape, generator=gen, device=DEV) * scale).float()


def _operands(N, K, nS, ldb, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    W = _rand(N, K, scale=K ** -0.5, gen=g)
    Wb = torch.zeros(N, (K + 31) // 32 * 32, dtype=torch.bfloat16, device=DEV)
    Wb[:, :K].copy_(W)
    X = torch.zeros(K, ldb, device=DEV)
    X[:, :nS] = _elu(_rand(K, nS, gen=g).double()).float()   # (an ELU activation, as the hidden layers see; padding columns 0)
    return W, Wb, X, g


SHAPES = [(512, 512, 1024, 1024), (512, 512, 8192, 8192), (512, 512, 65536, 65536), (512, 512, 1000, 1152), (256, 384, 4096, 4096)]


@pytest.mark.parametrize("N,K,nS,ldb", SHAPES)
def test_forward_against_exact_emulation(N, K, nS, ldb):
    W, Wb, X, g = _operands(N, K, nS, ldb, 1)
    bias = _rand(N, scale=0.1, gen=g)
    Y = torch.full((N, ldb), 12345.0, device=DEV)
    ops.linear_bf16_fwd(Wb[:, :K], bias, X, Y, nS, _lib.NIC_ACT_ELU)
    nc = (nS + 3) // 4 * 4
    ref, tol = emu.forward(W, X[:, :nc], bias)   # accumulation + bias add + the ELU's approximation
    _within(Y[:, :nc], ref, tol, "forward")
    # padding columns: as the FP32 kernel leaves them
    Yf = torch.full((N, ldb), 12345.0, device=DEV)
    ops.linear_fwd(W, bias, X, Yf, nS, _lib.NIC_ACT_ELU)
    assert torch.equal(Y[:, nc:], Yf[:, nc:])
    # identity activation, no bias
    Y2 = torch.empty(N, ldb, device=DEV)
    ops.linear_bf16_fwd(Wb[:, :K], None, X, Y2, nS, _lib.NIC_ACT_NONE)
    ref, tol = emu.forward(W, X[:, :nc], None, act_elu=False)
    _within(Y2[:, :nc], ref, tol, "forward (no bias, identity)")


@pytest.mark.parametrize("N,K,nS,ldb", SHAPES)
@pytest.mark.parametrize("accumulate", [0, 1])
def test_dgrad_against_exact_emulation(N, K, nS, ldb, accumulate):
    # dX[K][b] = (Wt[K][N] dY[N][b]) * ELU'(H[K][b]) (+ dX)
    W, _, _, g = _operands(N, K, 8, 8, 2)
    Wtb = torch.zeros(K, (N + 31) // 32 * 32, dtype=torch.bfloat16, device=DEV)
    Wtb[:, :N].copy_(W.t())
    dY = torch.zeros(N, ldb, device=DEV)
    dY[:, :nS] = _rand(N, nS, scale=1e-3, gen=g)
    H = _elu(_rand(K, ldb, gen=g).double()).float()
    prev = _rand(K, ldb, scale=1e-3, gen=g)
    dX = prev.clone()
    ops.linear_bf16_dgrad(Wtb[:, :N], dY, H, dX, nS, _lib.NIC_ACT_ELU, accumulate)
    nc = (nS + 3) // 4 * 4
    ref, tol = emu.dgrad(W.t(), dY[:, :nc], H[:, :nc], prev[:, :nc] if accumulate else None)
    _within(dX[:, :nc], ref, tol, "dgrad")
    assert torch.equal(dX[:, nc:], prev[:, nc:])   # (the FP32 kernel writes columns < round_up(n, 4) only, too)


@pytest.mark.parametrize("N,K,nS,ldb", [(512, 512, 1024, 1024), (512, 512, 8192, 8192), (512, 512, 1000, 1152), (256, 384, 4096, 4096)])
def test_wgrad_against_exact_emulation(N, K, nS, ldb):
    g = torch.Generator(device=DEV).manual_seed(3)
    dY = _rand(N, ldb, scale=1e-3, gen=g)   # (padding columns hold garbage: they must not count)
    X = _rand(K, ldb, gen=g)
    splits = ops.wgrad_num_splits(N, K, nS)
    slab = torch.zeros(splits, N, (K + 1 + 3) // 4 * 4, device=DEV)
    ops.linear_bf16_wgrad(dY, X, slab, nS)
    ops.linear_bf16_wgrad(dY, X, slab, nS)   # (a second period adds to the slab)
    gw, gb = torch.empty(N, K, device=DEV), torch.empty(N, device=DEV)
    ops.wgrad_reduce(slab, gw, gb, K, 1.0)
    ref, tol, ref_b, tol_b = emu.wgrad(dY[:, :nS], X[:, :nS], repeats=2)
    _within(gw, ref, tol, "wgrad")
    _within(gb, ref_b, tol_b, "bias gradient")


@pytest.mark.parametrize("nS,ldb", [(1024, 1024), (1000, 1152)])
def test_wgrad_periods_against_exact_emulation(nS, ldb):
    # T = 7 periods; histories whose period strides are not the matrices' sizes ([T][N + 5][ldb] and [T][K + 3][ldb])
    N, K, T = 512, 512, 7
    g = torch.Generator(device=DEV).manual_seed(4)
    dYh = _rand(T, N + 5, ldb, scale=1e-3, gen=g)
    Xh = _rand(T, K + 3, ldb, gen=g)
    splits = ops.wgrad_periods_num_splits(N, K, nS, T)
    slab = torch.zeros(splits, N, (K + 1 + 3) // 4 * 4, device=DEV)
    ops.linear_bf16_wgrad_periods(dYh[:, :N], Xh[:, :K], slab, nS)
    gw, gb = torch.empty(N, K, device=DEV), torch.empty(N, device=DEV)
    ops.wgrad_reduce(slab, gw, gb, K, 1.0)
    ref, tol, ref_b, tol_b = emu.wgrad_periods(dYh[:, :N, :nS], Xh[:, :K, :nS])
    _within(gw, ref, tol, "wgrad over periods")
    _within(gb, ref_b, tol_b, "bias gradient over periods")
    # determinism: the same launch again gives the same bits
    slab2 = torch.zeros_like(slab)
    ops.linear_bf16_wgrad_periods(dYh[:, :N], Xh[:, :K], slab2, nS)
    assert torch.equal(slab, slab2)


def test_kernels_deterministic():
    N, K, nS, ldb = 512, 512, 8192, 8192
    W, Wb, X, g = _operands(N, K, nS, ldb, 5)
    bias = _rand(N, gen=g)
    outs = []
    for _ in range(2):
        Y = torch.zeros(N, ldb, device=DEV)
        ops.linear_bf16_fwd(Wb[:, :K], bias, X, Y, nS, _lib.NIC_ACT_ELU)
        dX = torch.zeros(K, ldb, device=DEV)
        ops.linear_bf16_dgrad(Wb[:, :K], Y, X, dX, nS, _lib.NIC_ACT_ELU, 0)
        slab = torch.zeros(ops.wgrad_num_splits(N, K, nS), N, K + 4, device=DEV)
        ops.linear_bf16_wgrad(Y, X, slab, nS)
        outs.append((Y, dX, slab))
    for a, b in zip(*outs):
        assert torch.equal(a, b)


# ---- the shape sweep: everything nic_linear_bf16_ok admits, not only multiples of 128 ------------------------------------------
# Every case: NaN-filled outputs (with guard rows behind them), random garbage in every input column at or beyond
# round_up(n, 4) (the weight gradient: beyond n), zeros in [n, round_up(n, 4)) as the engine keeps them, an ldb well above
# round_up(n, 4), and weights that are a view into a wider bf16 buffer (row stride K + 40, a multiple of 8, garbage around them).
# The bounds are tests/bf16_emulation.py's (tests/test_bf16_emulation_host.py shows what they catch); each test prints its worst
# error / bound and the case it came from.  Measured on MI355X: DESIGN.md section 11.

SWEEP_NK = [(128, 128), (160, 224), (288, 160), (512, 160), (224, 512)]
SWEEP_N_WX = [1, 3, 4, 5, 33, 63, 64, 65, 1000]
SWEEP_N_WGRAD = [1, 31, 100, 1001, 4099]
NAN = float("nan")


def _r4(n):
    return (n + 3) // 4 * 4


def _last_kernel():
    return _lib.lib().nic_last_kernel().decode()


def _cu_count():
    """the library's CU count (nic::cu_count(): the device's multiprocessor count)"""
    return torch.cuda.get_device_properties(torch.device(DEV)).multi_processor_count


def _wide_bf16(W, g):
    """bf16(W) as a view into a wider buffer: row stride K + 40, first column 8 (16-byte aligned), garbage everywhere else"""
    rows, cols = W.shape
    buf = _rand(rows, cols + 40, scale=100.0, gen=g).to(torch.bfloat16)
    view = buf[:, 8:8 + cols]
    view.copy_(W)
    assert view.stride(0) == cols + 40 and view.data_ptr() % 16 == 0
    return view


def _activations(rows, n, ldb, g, scale=None, zero_to=None):
    """[rows][ldb]: data in columns < n (an ELU activation, or scale * N(0, 1)), zeros up to `zero_to`, garbage behind"""
    t = _rand(rows, ldb, scale=50.0, gen=g)
    data = _rand(rows, n, gen=g)
    t[:, :n] = _elu(data.double()).float() if scale is None else data * scale
    t[:, n:zero_to if zero_to is not None else n] = 0.0
    return t


def _nan_out(rows, ldb, guard=3):
    buf = torch.full((rows + guard, ldb), NAN, device=DEV)
    return buf, buf[:rows]


def _all_nan(t):
    return bool(torch.isnan(t).all())


def _forward_case(N, K, n, seed):
    """one forward launch with bias + ELU and one without: (worst ratio, kernel name)"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    nc = _r4(n)
    ldb = nc + 72
    W = _rand(N, K, scale=K ** -0.5, gen=g)
    Wv = _wide_bf16(W, g)
    X = _activations(K, n, ldb, g, zero_to=nc)
    bias = _rand(N, scale=0.1, gen=g)
    worst = 0.0
    for b, act in ((bias, _lib.NIC_ACT_ELU), (None, _lib.NIC_ACT_NONE)):
        buf, Y = _nan_out(N, ldb)
        ops.linear_bf16_fwd(Wv, b, X, Y, n, act)
        kernel = _last_kernel()
        ref, tol = emu.forward(W, X[:, :nc], b, act_elu=act == _lib.NIC_ACT_ELU)
        worst = max(worst, _within(Y[:, :nc], ref, tol, f"forward {N}x{K}, n={n}, act={act} ({kernel})"))
        assert _all_nan(Y[:, nc:]) and _all_nan(buf[N:]), f"forward {N}x{K}, n={n}: wrote beyond round_up(n, 4) or beyond row N"
    return worst, kernel


def _dgrad_case(N, K, n, seed):
    """dgrad with ELU' and without an activation (Hprev = None), with and without accumulate: (worst ratio, kernel name)"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    nc = _r4(n)
    ldb = nc + 72
    Wt = _rand(K, N, scale=K ** -0.5, gen=g)
    Wtv = _wide_bf16(Wt, g)
    dY = _activations(N, n, ldb, g, scale=1e-3, zero_to=nc)
    H = _activations(K, nc, ldb, g)
    prev = _rand(K, nc, scale=1e-3, gen=g)
    worst = 0.0
    for h, act in ((H, _lib.NIC_ACT_ELU), (None, _lib.NIC_ACT_NONE)):
        for accumulate in (0, 1):
            buf, dX = _nan_out(K, ldb)
            if accumulate:
                dX[:, :nc] = prev
            ops.linear_bf16_dgrad(Wtv, dY, h, dX, n, act, accumulate)
            kernel = _last_kernel()
            ref, tol = emu.dgrad(Wt, dY[:, :nc], h[:, :nc] if h is not None else None, prev if accumulate else None)
            what = f"dgrad {N}x{K}, n={n}, act_prev={act}, accumulate={accumulate} ({kernel})"
            worst = max(worst, _within(dX[:, :nc], ref, tol, what))
            assert _all_nan(dX[:, nc:]) and _all_nan(buf[K:]), f"{what}: wrote beyond round_up(n, 4) or beyond row K"
    return worst, kernel


@pytest.mark.parametrize("N,K", SWEEP_NK)
def test_sweep_forward(N, K):
    worst = max((_forward_case(N, K, n, 100 + n) + (n,) for n in SWEEP_N_WX), key=lambda r: r[0])
    print(f"RATIO forward {N}x{K}: worst error / bound {worst[0]:.4f} at n={worst[2]} ({worst[1]})")


@pytest.mark.parametrize("N,K", SWEEP_NK)
def test_sweep_dgrad(N, K):
    worst = max((_dgrad_case(N, K, n, 200 + n) + (n,) for n in SWEEP_N_WX), key=lambda r: r[0])
    print(f"RATIO dgrad {N}x{K}: worst error / bound {worst[0]:.4f} at n={worst[2]} ({worst[1]})")


@pytest.mark.parametrize("N,K", [(160, 224), (288, 160)])
@pytest.mark.parametrize("entry", ["forward", "dgrad"])
def test_partial_row_tiles_in_both_tilings(entry, N, K):
    """Output rows that are no multiple of the tile height, in the 64 x 64 tiling (a small batch) and in the 128 x 128 tiling,
    which launch_wx takes from two row-tile x column-tile workgroups per CU: the column count is worked out from the CU count."""
    case, M, epi = (_forward_case, N, 0) if entry == "forward" else (_dgrad_case, K, 1)
    assert M % 128 != 0 and M % 64 != 0
    row_tiles = (M + 127) // 128
    col_tiles = (2 * _cu_count() + row_tiles - 1) // row_tiles
    n_big = 128 * col_tiles - 61
    for n, variant in ((1000, f"bf16_wx_kernel<1,1,{epi}>"), (n_big, f"bf16_wx_kernel<2,2,{epi}>")):
        worst, kernel = case(N, K, n, 300 + n)
        assert kernel == variant, (kernel, variant, n)
        print(f"RATIO {entry} {N}x{K}: worst error / bound {worst:.4f} at n={n} ({kernel}, {M} output rows)")


def _prefilled_slab(slots, N, lds):
    """a known pattern without zeros, small next to the sums (so that the bound's term for it stays small): 2^-16 * (1..7)"""
    i = torch.arange(slots * N * lds, device=DEV)
    return (((i % 7) + 1).float() * 2.0 ** -16 * (1 - 2 * (i % 2)).float()).view(slots, N, lds)


def _check_slab(slab, before, owned, K, ref, tol, ref_b, tol_b, what):
    """slab - before, summed over the slots, against the emulation; slots outside `owned` and the columns beyond K + 1 bit-identical"""
    for s in range(slab.shape[0]):
        if s not in owned:
            assert torch.equal(slab[s], before[s]), f"{what}: slot {s} is not the launch's, but it changed"
    assert torch.equal(slab[:, :, K + 1:], before[:, :, K + 1:]), f"{what}: slab columns beyond K + 1 changed"
    delta = (slab.double() - before.double()).sum(0)
    return max(_within(delta[:, :K], ref, tol, what), _within(delta[:, K], ref_b, tol_b, what + ", bias column"))


@pytest.mark.parametrize("N,K", SWEEP_NK)
def test_sweep_wgrad(N, K):
    lds = _r4(K + 1) + 4
    worst, many = (0.0, None), 0.0
    for n in SWEEP_N_WGRAD:
        g = torch.Generator(device=DEV).manual_seed(400 + n)
        ldb = _r4(n) + 72
        dY = _activations(N, n, ldb, g, scale=1e-3)   # (garbage from column n on: it must not count)
        X = _activations(K, n, ldb, g, scale=1.0)
        for slots in (1, 3, 64):
            before = _prefilled_slab(slots, N, lds)
            slab = before.clone()
            ops.linear_bf16_wgrad(dY, X, slab, n)
            assert _last_kernel() == "bf16_wgrad_kernel<2,2>"
            # slots the launch owns (wgrad_bf16 in csrc/linear_bf16.hip): chunks of round_up(ceil(n / slots), 32) scenarios
            chunk = ((n + slots - 1) // slots + 31) // 32 * 32
            owned = {s for s in range(slots) if s * chunk < n}
            ref, tol, ref_b, tol_b = emu.wgrad(dY[:, :n], X[:, :n], base_w=before[:, :, :K].abs().amax(0),
                                               base_b=before[:, :, K].abs().amax(0))
            r = _check_slab(slab, before, owned, K, ref, tol, ref_b, tol_b, f"wgrad {N}x{K}, n={n}, {slots} slots")
            worst = max(worst, (r, f"n={n}, {slots} slots ({len(owned)} owned)"))
            many = max(many, r if n > 1 else 0.0)
    # (n = 1 into a pre-filled slab: ONE rounding of base + product, which is what the bound allows - a ratio just below 1)
    print(f"RATIO wgrad {N}x{K}: worst error / bound {worst[0]:.4f} at {worst[1]}; from 31 scenarios up {many:.4f}")


def _period_factors(n_slots, n, T):
    """`period_factors` / `wgrad_flush_periods` of csrc/wgrad_plan.h (what `wgrad_bf16` of csrc/linear_bf16.hip launches with)
    restated: (scenario splits, period groups, chunk, periods per
    group, flush).  It CHOOSES the cases below and names the slots a launch owns; no numerical result is judged by it."""
    ss = max(1, min(n_slots, max(1, n // 128)))
    groups = max(1, min(n_slots // ss, T))
    chunk = ((n + ss - 1) // ss + 31) // 32 * 32
    return ss, groups, chunk, (T + groups - 1) // groups, max(1, 8192 // chunk)


# (slots, n, T, N, K, what the case is there for, a check of the restated factors that says so)
PERIOD_CASES = [
    (2, 4096, 11, 160, 224, "flush segments of 4 + 4 + 3 periods", lambda ss, g, chunk, ppg, flush: (ss, g, chunk, ppg, flush) == (2, 1, 2048, 11, 4)),
    (4, 4099, 9, 288, 160, "segments of 7 + 2 periods, ragged chunks", lambda ss, g, chunk, ppg, flush: (ss, g, chunk, ppg, flush) == (4, 1, 1056, 9, 7)),
    (1, 8203, 3, 160, 224, "flush == 1 (chunk >= 8,192): a segment per period", lambda ss, g, chunk, ppg, flush: chunk >= 8192 and flush == 1 and ppg == 3),
    (6, 300, 7, 160, 224, "3 period groups of 3 + 3 + 1 periods", lambda ss, g, chunk, ppg, flush: (ss, g, ppg) == (2, 3, 3)),
    (4, 100, 5, 128, 128, "4 groups x 2 periods over T = 5: the last group idle", lambda ss, g, chunk, ppg, flush: (ss, g, ppg) == (1, 4, 2)),
    (7, 300, 2, 288, 160, "7 slots, 2 x 2 used", lambda ss, g, chunk, ppg, flush: ss * g == 4),
    (3, 1001, 1, 224, 512, "T = 1", lambda ss, g, chunk, ppg, flush: (ss, g, ppg) == (3, 1, 1)),
    (64, 100, 13, 512, 160, "64 slots at 100 scenarios: 13 groups of one period", lambda ss, g, chunk, ppg, flush: (ss, g, ppg) == (1, 13, 1)),
]


@pytest.mark.parametrize("slots,n,T,N,K,why,expect", PERIOD_CASES, ids=[c[5] for c in PERIOD_CASES])
def test_wgrad_periods_slot_splits_and_flush_segments(slots, n, T, N, K, why, expect):
    ss, groups, chunk, ppg, flush = _period_factors(slots, n, T)
    assert expect(ss, groups, chunk, ppg, flush), (why, ss, groups, chunk, ppg, flush)
    g = torch.Generator(device=DEV).manual_seed(500 + n + T)
    ldb, lds = _r4(n) + 72, _r4(K + 1) + 4
    # histories whose period strides are not the matrices' sizes; garbage from column n on
    dYh = torch.stack([_activations(N + 5, n, ldb, g, scale=1e-3) for _ in range(T)])
    Xh = torch.stack([_activations(K + 3, n, ldb, g, scale=1.0) for _ in range(T)])
    owned = {grp * ss + s for grp in range(groups) for s in range(ss) if s * chunk < n and grp * ppg < T}
    before = _prefilled_slab(slots, N, lds)
    slabs = []
    for _ in range(2):   # twice into fresh slabs: the same bits
        slab = before.clone()
        ops.linear_bf16_wgrad_periods(dYh[:, :N], Xh[:, :K], slab, n)
        slabs.append(slab)
    assert torch.equal(slabs[0], slabs[1])
    ref, tol, ref_b, tol_b = emu.wgrad_periods(dYh[:, :N, :n], Xh[:, :K, :n], base_w=before[:, :, :K].abs().amax(0),
                                               base_b=before[:, :, K].abs().amax(0))
    r = _check_slab(slabs[0], before, owned, K, ref, tol, ref_b, tol_b, f"wgrad over periods ({why})")
    # the tile scan (tests/bf16_emulation.py): with T * n terms the dense bound above no longer shows ONE lost or doubled
    # 32-scenario tile, so the same launch runs m more times on |dY| with every m-th (period, tile) kept - each tile once
    m = emu.tile_scan_stride(T * n)
    r_scan = 0.0
    if m > 1:
        dYa, Xa = dYh.abs(), Xh.abs()
        for rr in range(m):
            mask = emu.tile_mask(T, n, ldb, m, rr, DEV)[:, None, :]
            dYm = torch.where(mask, dYa, torch.zeros_like(dYa))
            dYm[:, :, n:] = dYh[:, :, n:]   # (the garbage behind column n stays)
            slab = torch.zeros(slots, N, lds, device=DEV)
            ops.linear_bf16_wgrad_periods(dYm[:, :N], Xa[:, :K], slab, n)
            ref, tol, ref_b, tol_b = emu.wgrad_periods(dYm[:, :N, :n], Xa[:, :K, :n])
            what = f"wgrad over periods ({why}), tile scan pass {rr} of {m}"
            r_scan = max(r_scan, _check_slab(slab, torch.zeros_like(slab), owned, K, ref, tol, ref_b, tol_b, what))
    segments = [min(flush, ppg - p) for p in range(0, ppg, flush)]
    print(f"RATIO wgrad_periods {N}x{K}: worst error / bound {r:.4f} (tile scan, {m} passes: {r_scan:.4f}) at {slots} slots, "
          f"n={n}, T={T}: {why}; {ss} scenario splits x {groups} period groups, chunk {chunk}, flush segments of {segments} "
          f"periods, {len(owned)} slots owned")


# ---- special values ------------------------------------------------------------------------------------------------------------
FLT_MAX = 3.4028234663852886e38   # rounds to +Inf in bf16
DENORM = 2.0 ** -127              # an FP32 denormal that is a bf16 denormal as well (so are its small multiples)


def _special_check(got, ref, tol, clean_rows, clean_cols, what):
    """NaN and +-Inf exactly where the emulation has them, the bound everywhere else; the clean rows x columns all finite"""
    got = got.double().cpu()
    assert torch.equal(torch.isnan(got), torch.isnan(ref)), f"{what}: NaN pattern differs from the emulation's"
    inf = torch.isinf(ref)
    assert torch.equal(torch.isinf(got), inf) and torch.equal(got[inf], ref[inf]), f"{what}: +-Inf pattern differs"
    fin = torch.isfinite(ref)
    assert bool(torch.isfinite(got[clean_rows][:, clean_cols]).all()), f"{what}: a special value reached a clean row / column"
    assert int(fin.sum()) >= len(clean_rows) * len(clean_cols)
    return _within(got[fin], ref[fin], tol[fin], what)


def test_special_values_forward():
    """+-Inf, NaN, the largest finite float, FP32 denormals and -0.0 in a few scenario columns of X (converted on the device) and
    a few weight rows (converted by torch): each must stay in its column / row, as in the emulation (evaluated on the CPU).
    Column 150 of X holds ONLY denormals and weight row 70 is scaled by 2^100: output (70, 150) is an exact sum of products near
    2^-24 - a conversion (or an MFMA operand path) that flushes denormals gives 0 there, far outside the bound.  No bias and no
    activation, so that nothing hides them."""
    N, K, n = 160, 224, 200
    g = torch.Generator(device=DEV).manual_seed(600)
    ldb = _r4(n) + 72
    W = _rand(N, K, scale=K ** -0.5, gen=g)
    X = _activations(K, n, ldb, g, zero_to=_r4(n))
    inf = float("inf")
    for (k, b), v in {(3, 5): inf, (10, 17): -inf, (0, 40): NAN, (100, 77): FLT_MAX, (3, 99): inf, (4, 99): -inf, (7, 130): 1e-40,
                      (8, 130): -0.0, (9, 131): -FLT_MAX}.items():
        X[k, b] = v
    X[:, 150] = DENORM * (1 + torch.arange(K, device=DEV) % 3).float() * (1 - 2 * (torch.arange(K, device=DEV) % 2)).float()
    x_cols = {5, 17, 40, 77, 99, 130, 131}
    for (r, k), v in {(20, 50): inf, (33, 1): NAN, (47, 60): FLT_MAX, (60, 20): -0.0, (60, 21): 1e-40, (61, 22): -inf}.items():
        W[r, k] = v
    w_rows = {20, 33, 47, 61}
    W[70] *= 2.0 ** 100   # (row 70: denormal x 2^100 - sums near 2^-24, far above the bound's 1e-30 floor, exact products)
    Wv = _wide_bf16(W, g)
    buf, Y = _nan_out(N, ldb)
    ops.linear_bf16_fwd(Wv, None, X, Y, n, _lib.NIC_ACT_NONE)
    ref, tol = emu.forward(W.cpu(), X[:, :n].cpu(), None, act_elu=False)
    clean_rows = [r for r in range(N) if r not in w_rows]
    clean_cols = [b for b in range(n) if b not in x_cols]
    r = _special_check(Y[:, :n], ref, tol, clean_rows, clean_cols, "forward with special values")
    assert 150 in clean_cols and 70 in clean_rows and 1e-12 < abs(float(ref[70, 150])) and float(tol[70, 150]) < 1e-3 * abs(float(ref[70, 150]))
    assert _all_nan(Y[:, _r4(n):]) and _all_nan(buf[N:])
    print(f"RATIO forward special values: worst error / bound over the finite outputs {r:.4f}")


def test_special_values_wgrad():
    """The same values in dY and X of the weight gradient (both converted on the device), 3 slots over 200 scenarios: a special
    value in scenario b of row n of dY reaches row n of the slab (and its bias column) only, one in row k of X column k only.
    Row 55 of X holds only denormals (judged at row 70 of dY, scaled by 2^110).  The bias column is an FP32 sum of the unrounded dY: the largest finite float stays finite."""
    N, K, n, slots = 160, 224, 200, 3
    g = torch.Generator(device=DEV).manual_seed(601)
    ldb, lds = _r4(n) + 72, _r4(K + 1) + 4
    dY = _activations(N, n, ldb, g, scale=1e-3)
    X = _activations(K, n, ldb, g, scale=1.0)
    inf = float("inf")
    for (r, b), v in {(5, 10): inf, (12, 100): NAN, (20, 50): FLT_MAX, (25, 60): 1e-40, (26, 61): -0.0, (30, 199): -inf}.items():
        dY[r, b] = v
    for (k, b), v in {(30, 150): -inf, (40, 195): FLT_MAX, (50, 61): -0.0, (51, 62): 1e-40, (60, 3): NAN}.items():
        X[k, b] = v
    X[55, :n] = DENORM * (1 + torch.arange(n, device=DEV) % 3).float() * (1 - 2 * (torch.arange(n, device=DEV) % 2)).float()
    dy_rows, x_rows = {5, 12, 20, 30}, {30, 40, 60}
    dY[70, :n] *= 2.0 ** 110   # (row 70 x the denormal row 55: a sum near 2^-24, far above the bound's 1e-30 floor)
    slab = torch.zeros(slots, N, lds, device=DEV)
    ops.linear_bf16_wgrad(dY, X, slab, n)
    ref, tol, ref_b, tol_b = emu.wgrad(dY[:, :n].cpu(), X[:, :n].cpu())
    got = slab.double().sum(0).cpu()
    clean_rows = [r for r in range(N) if r not in dy_rows]
    clean_cols = [k for k in range(K) if k not in x_rows]
    r = _special_check(got[:, :K], ref, tol, clean_rows, clean_cols, "wgrad with special values")
    assert 1e-12 < abs(float(ref[70, 55])) and float(tol[70, 55]) < 1e-3 * abs(float(ref[70, 55]))
    rb = _special_check(got[:, K:K + 1], ref_b[:, None], tol_b[:, None], clean_rows, [0], "bias gradient with special values")
    assert bool(torch.isfinite(got[20, K])) and bool((got[:, K + 1:] == 0).all())
    print(f"RATIO wgrad special values: worst error / bound over the finite outputs {max(r, rb):.4f}")


# ---- argument refusal: an error through _lib.check, no launch, the output as it was ----------------------------------------------

def _refused(call, out, message):
    """`call` must raise NicError naming `message`, launch nothing (the last launched kernel stays the marker launch made here)
    and leave `out` bit-identical"""
    marker = torch.zeros(8, 8, device=DEV)
    ops.round_orders(marker, 8)
    launched = _last_kernel()
    assert "bf16" not in launched
    before = out.clone()
    with pytest.raises(_lib.NicError, match=message):
        call()
    torch.cuda.synchronize()
    assert _last_kernel() == launched, "a refused call launched a kernel"
    assert torch.equal(out.view(torch.int32), before.view(torch.int32)), "a refused call changed its output"


def _off_by_4_bytes(rows, ldb, fill=0.0):
    """a [rows][ldb] FP32 view that starts 4 bytes behind a 16-byte boundary"""
    buf = torch.full((rows * ldb + 4,), fill, device=DEV)
    view = buf[1:1 + rows * ldb].view(rows, ldb)
    assert view.data_ptr() % 16 == 4
    return view


def test_bf16_entry_points_refuse_bad_arguments():
    n, ldb = 100, 128
    bz = lambda r, c, ld=None: torch.zeros(r, ld or c, dtype=torch.bfloat16, device=DEV)[:, :c]   # noqa: E731
    fz = lambda r, c=ldb: torch.ones(r, c, device=DEV)   # noqa: E731
    out = lambda r, c=ldb: torch.full((r, c), NAN, device=DEV)   # noqa: E731
    ELU, NONE = _lib.NIC_ACT_ELU, _lib.NIC_ACT_NONE
    shape = "multiples of 32"
    # -- forward: Y[N][ldb] = W[N][K] X[K][ldb]
    fwd = lambda W, X, Y, nn=n: (lambda: ops.linear_bf16_fwd(W, None, X, Y, nn, ELU))   # noqa: E731
    Y = out(128)
    for N, K in ((96, 128), (128, 130), (144, 128)):
        Yn = out(N)
        _refused(fwd(bz(N, K, K + 6 if K % 8 else None), fz(K), Yn), Yn, shape)
    _refused(fwd(bz(128, 128, 132), fz(128), Y), Y, "multiple of 8")
    _refused(fwd(bz(128, 128), _off_by_4_bytes(128, ldb, 1.0), Y), Y, "16-byte aligned")
    Yo = _off_by_4_bytes(128, ldb, NAN)
    _refused(fwd(bz(128, 128), fz(128), Yo), Yo, "16-byte aligned")
    Y64 = out(128, 64)
    _refused(fwd(bz(128, 128), fz(128, 64), Y64), Y64, "n_scenarios")   # ldb = 64 < n = 100
    _refused(fwd(bz(128, 128), fz(128), Y, 0), Y, "n_scenarios")
    Y130 = out(128, 130)
    _refused(fwd(bz(128, 128), fz(128, 130), Y130), Y130, "multiple of 4")
    with pytest.raises(TypeError):
        ops.linear_bf16_fwd(torch.zeros(128, 128, device=DEV), None, fz(128), Y, n, ELU)
    # -- dgrad: dX[K][ldb] = Wt[K][N] dY[N][ldb]
    dgr = lambda Wt, dY, dX, nn=n: (lambda: ops.linear_bf16_dgrad(Wt, dY, None, dX, nn, NONE, 0))   # noqa: E731
    dX = out(128)
    for N, K in ((96, 128), (128, 130), (144, 128)):
        dXk = out(K)
        _refused(dgr(bz(K, N), fz(N), dXk), dXk, shape)
    _refused(dgr(bz(128, 128, 132), fz(128), dX), dX, "multiple of 8")
    _refused(dgr(bz(128, 128), _off_by_4_bytes(128, ldb, 1.0), dX), dX, "16-byte aligned")
    dXo = _off_by_4_bytes(128, ldb, NAN)
    _refused(dgr(bz(128, 128), fz(128), dXo), dXo, "16-byte aligned")
    dX64 = out(128, 64)
    _refused(dgr(bz(128, 128), fz(128, 64), dX64), dX64, "n_scenarios")
    _refused(dgr(bz(128, 128), fz(128), dX, 0), dX, "n_scenarios")
    dX130 = out(128, 130)
    _refused(dgr(bz(128, 128), fz(128, 130), dX130), dX130, "multiple of 4")
    with pytest.raises(TypeError):
        ops.linear_bf16_dgrad(torch.zeros(128, 128, device=DEV), fz(128), None, dX, n, NONE, 0)
    # -- weight gradients: slab[slots][N][lds] += dY[N][ldb] X[K][ldb]^T
    slab = lambda N, K: torch.full((2, N, K + 4), NAN, device=DEV)   # noqa: E731
    for name, wg in (("single period", lambda dY, X, s, nn=n: (lambda: ops.linear_bf16_wgrad(dY, X, s, nn))),
                     ("over periods", lambda dY, X, s, nn=n: (lambda: ops.linear_bf16_wgrad_periods(dY[None], X[None], s, nn)))):
        for N, K in ((96, 128), (128, 130), (144, 128)):
            s = slab(N, K)
            _refused(wg(fz(N), fz(K), s), s, shape)
        s = slab(128, 128)
        _refused(wg(_off_by_4_bytes(128, ldb, 1.0), fz(128), s), s, "16-byte aligned")
        _refused(wg(fz(128), _off_by_4_bytes(128, ldb, 1.0), s), s, "16-byte aligned")
        _refused(wg(fz(128, 64), fz(128, 64), s), s, "n_scenarios")
        _refused(wg(fz(128), fz(128), s, 0), s, "n_scenarios")
        _refused(wg(fz(128, 130), fz(128, 130), s), s, "multiple of 4")
    # -- over periods: no periods; a period stride that is no multiple of 4 elements
    s = slab(128, 128)
    hist = torch.ones(3 * (128 * ldb + 2), device=DEV)
    odd = hist.as_strided((3, 128, ldb), (128 * ldb + 2, ldb, 1))
    even = torch.ones(3, 128, ldb, device=DEV)
    _refused(lambda: ops.linear_bf16_wgrad_periods(odd, even, s, n), s, "period strides")
    _refused(lambda: ops.linear_bf16_wgrad_periods(even, odd, s, n), s, "period strides")
    lib, st = _lib.lib(), _lib.current_stream()
    _refused(lambda: _lib.check(lib.nic_linear_bf16_wgrad_periods(even.data_ptr(), even.data_ptr(), s.data_ptr(), s.stride(1), 128, 128,
                                                                  n, ldb, 2, 0, 128 * ldb, 128 * ldb, st)), s, "n_periods")


# ---- the engine ------------------------------------------------------------------------------------------------------------------

def _case(workload, n, T, seed=7):
    setting, policy, _, _, _ = workloads.get(workload)
    obs = defaultdict(lambda: None, setting["observation_params"])
    sc = Scenario(T, setting["problem_params"], setting["store_params"], setting["warehouse_params"], setting["echelon_params"], n,
                  obs, setting["seeds"], sampler="hip", device=DEV)
    data = {k: v.to(DEV) for k, v in sc.get_data().items()}
    torch.manual_seed(seed)
    model = NeuralNetworkCreator().create_neural_network(sc, policy, device=DEV)
    eng = FusedRollout(model, setting["problem_params"], DEV)
    eng.materialize(eng.input_rows(data, obs))
    return setting, data, model, eng, obs


def _engine(model, setting, data, obs, precision=None, **opts):
    eng = FusedRollout(model, setting["problem_params"], DEV)
    eng.materialize(eng.input_rows(data, obs))
    if precision is not None:
        eng.gemm_precision = precision
    for k, v in opts.items():
        setattr(eng, k, v)
    return eng


def _train(eng, data, T, obs):
    total, _ = eng.run(data, T, 0, train=True, observation_params=obs, assign_grads=False)
    torch.cuda.synchronize()
    return total.clone(), [g.clone() for _, g in eng.param_grads()]


def _hidden_512(model):
    lins = model.master_linears()
    return [i for i in range(1, len(lins) - 1) if lins[i].in_features == 512 and lins[i].out_features == 512]


@pytest.mark.parametrize("workload,n,T,route", [("cfg3", 1024, 10, "tail"), ("cfg3", 32768, 4, "per-period"), ("cfg5", 1024, 4, "any")])
def test_rollout_bf16_against_fp32(workload, n, T, route):
    """bf16 mode against the FP32 engine, same weights and batch.  The bars (total 5e-3 relative, per-parameter gradient cosine
    >= 0.98 and |dg| / |g| <= 0.2) were set from bf16's 2^-8 relative step before anything was measured.  Measured on MI355X at
    the initial weights: batch total within 1.0e-5 (cfg3, 1,024 x T=10), 1.9e-6 (cfg3, 32,768 x T=4), 2.7e-4 (cfg5, 1,024 x T=4);
    every gradient tensor cosine >= 0.99997 and |dg| / |g| = 0.003-0.008."""
    setting, data, model, _, obs = _case(workload, n, T)
    fp = _engine(model, setting, data, obs)
    bf = _engine(model, setting, data, obs, "bf16")
    t_fp, g_fp = _train(fp, data, T, obs)
    t_bf, g_bf = _train(bf, data, T, obs)
    assert bf.bf16_layers == _hidden_512(model) and len(bf.bf16_layers) == 2
    assert fp.bf16_layers == []
    if route == "tail":
        assert bf._use_tail() and bf._use_tail_bwd()
    elif route == "per-period":
        assert not bf._use_tail()
    rel = abs(float(t_bf) - float(t_fp)) / abs(float(t_fp))
    stats = {"total_rel": rel}
    assert rel <= 5e-3, stats
    for k, (a, b) in enumerate(zip(g_fp, g_bf)):
        a, b = a.double().flatten(), b.double().flatten()
        cos = float(a @ b / (a.norm() * b.norm()).clamp_min(1e-300))
        dn = float((a - b).norm() / a.norm().clamp_min(1e-300))
        stats[f"g{k}"] = (round(cos, 5), round(dn, 4))
        assert cos >= 0.98 and dn <= 0.2, stats
    e_fp, _ = fp.run(data, T, 0, train=False, observation_params=obs)
    e_bf, _ = bf.run(data, T, 0, train=False, observation_params=obs)
    assert bf.bf16_layers == _hidden_512(model)
    assert abs(float(e_bf) - float(e_fp)) <= 5e-3 * abs(float(e_fp))
    print(f"{workload} {n}x{T}: {stats}")


def test_bf16_training_step_deterministic():
    setting, data, model, _, obs = _case("cfg3", 1024, 4)
    eng = _engine(model, setting, data, obs, "bf16")
    t1, g1 = _train(eng, data, 4, obs)
    t2, g2 = _train(eng, data, 4, obs)
    assert torch.equal(t1, t2) and all(torch.equal(a, b) for a, b in zip(g1, g2))


def test_graph_replay_matches_eager_in_bf16():
    """use_graph=True against eager, three training steps with Adam steps in between: the bf16 weight copies are refreshed in place
    before every replay, so the replayed steps see the moved weights (bit-identical totals and gradients)."""
    setting, data, model, _, obs = _case("cfg3", 1024, 4)
    model2 = copy.deepcopy(model)
    runs = []
    for m, graph in ((model, False), (model2, True)):
        # (fuse_tail=True: the same backward launches in both modes; "auto" picks the per-layer ones under replay at 1,024)
        eng = _engine(m, setting, data, obs, "bf16", use_graph=graph, fuse_tail=True)
        opt = torch.optim.Adam(m.parameters(), lr=1e-3)
        seq = []
        for _ in range(3):
            opt.zero_grad()
            total, _ = eng.run(data, 4, 0, train=True, observation_params=obs)
            torch.cuda.synchronize()
            seq.append((total.clone(), [p.grad.clone() for p in m.parameters()]))
            opt.step()
        if graph:
            assert set(eng._graphs) == {"fwd", "bwd"}
        runs.append(seq)
    for (ta, ga), (tb, gb) in zip(*runs):
        assert torch.equal(ta, tb)
        assert all(torch.equal(a, b) for a, b in zip(ga, gb))


def test_no_eligible_layers_and_explicit_fp32_unchanged():
    # cfg1: the small whole-horizon route (32-wide policy) - bf16 changes nothing
    setting, data, model, _, obs = _case("cfg1", 256, 8)
    a = _engine(model, setting, data, obs, "fp32")
    b = _engine(model, setting, data, obs, "bf16")
    ta, ga = _train(a, data, 8, obs)
    tb, gb = _train(b, data, 8, obs)
    assert b.small is not None and b.bf16_layers == []
    assert torch.equal(ta, tb) and all(torch.equal(x, y) for x, y in zip(ga, gb))
    # cfg3 at 1,024 x T=4: explicit "fp32" is the default, bit for bit
    setting, data, model, _, obs = _case("cfg3", 1024, 4)
    a = _engine(model, setting, data, obs)
    b = _engine(model, setting, data, obs, "fp32")
    ta, ga = _train(a, data, 4, obs)
    tb, gb = _train(b, data, 4, obs)
    assert b.bf16_layers == []
    assert torch.equal(ta, tb) and all(torch.equal(x, y) for x, y in zip(ga, gb))


def test_invalid_precision_and_wide_route_refused():
    setting, data, model, _, obs = _case("cfg3", 1024, 2)
    eng = _engine(model, setting, data, obs, "fp16")
    with pytest.raises(ValueError):
        eng.run(data, 2, 0, train=True, observation_params=obs)
    eng = _engine(model, setting, data, obs, "bf16", use_wide=True)
    with pytest.raises(ValueError):
        eng.run(data, 2, 0, train=True, observation_params=obs)


def test_bf16_training_still_learns():
    """cfg3_yaml (the reference's shipped one-warehouse batch: 5 stores, batches of 1,024 x T=50): 40 epochs at each precision from
    the same initial weights and shuffling seed, then both final policies evaluated IN FP32 on the dev set.

    40, not 20: measured on MI355X (dev loss every 5 epochs, two shuffling seeds per precision), the dev loss falls from ~19 to
    ~5.4 between epochs 15 and 25, and at epoch 20 two FP32 runs that differ only in the shuffling seed stood at 6.77 and 9.78
    (bf16: 11.8 and 11.5) - a 1.02 bar there measures where each run is in that drop.  At epoch 40 all four runs are on the
    plateau: FP32 5.343 / 5.346, bf16 5.364 / 5.373 (ratio 1.004 / 1.005)."""
    setting, hyper, _ = workloads.get_epoch("cfg3_yaml")
    torch.manual_seed(11)
    c = main_run.build(setting, hyper, DEV)
    model, loaders, sim, pbd = c["model"], c["data_loaders"], c["simulator"], c["params_by_dataset"]
    pp, obs = c["problem_params"], c["observation_params"]
    lr = hyper["optimizer_params"]["learning_rate"]

    def dev_loss(tr):
        tr.gemm_precision = "fp32"
        _, rep = tr.do_one_epoch(None, loaders["dev"], PolicyLoss(), sim, model, pbd["dev"]["periods"], pp, obs, train=False,
                                 ignore_periods=pbd["dev"]["ignore_periods"])
        return rep

    from neural_inventory_control_amd.trainer import Trainer
    untrained = dev_loss(Trainer(device=DEV))   # (also materialises the lazy first layer)
    init = copy.deepcopy(model.state_dict())
    final = {}
    for precision in ("fp32", "bf16"):
        model.load_state_dict(init)
        opt = torch.optim.Adam(model.parameters(), lr=lr)
        tr = Trainer(device=DEV)
        tr.gemm_precision = precision
        torch.manual_seed(5)
        for _ in range(40):
            tr.do_one_epoch(opt, loaders["train"], PolicyLoss(), sim, model, pbd["train"]["periods"], pp, obs, train=True,
                            ignore_periods=pbd["train"]["ignore_periods"])
        if precision == "bf16":
            eng = tr._engines[(id(model), True)]
            assert eng.bf16_layers == _hidden_512(model)
        final[precision] = dev_loss(tr)
    print(f"dev loss: untrained {untrained}, fp32 {final['fp32']}, bf16 {final['bf16']}")
    assert final["fp32"] < untrained and final["bf16"] < untrained
    assert final["bf16"] <= 1.02 * final["fp32"]


# ---- the engine's bf16 layers, checked in place -----------------------------------------------------------------------------------

@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_engine_bf16_layers_in_place(graph):
    """cfg3's setting with hidden layers [256, 160, 288, 96] at 1,037 scenarios x T = 6 in bf16 mode: layers 1 (160 x 256) and
    2 (288 x 160) are eligible, layer 3 (96 x 288), the first and the logits layer are not.  Three training runs with an Adam step
    after the first two (with use_graph the third is a replay), then every bf16 launch of the LAST run is judged where it stands:
    the engine keeps each period's activations (hidden) and pre-activation gradients (dZhist), so each layer's output is compared
    with the exact emulation of the FP32 input the kernel saw - the bounds of tests/bf16_emulation.py, no recurrence in between.
    A stale Wb / Wtb copy, a wrong transpose or a history off by one period misses them by orders of magnitude."""
    n, T = 1037, 6
    setting, policy, _, _, _ = workloads.get("cfg3")
    policy = copy.deepcopy(policy)
    policy["neurons_per_hidden_layer"]["master"] = [256, 160, 288, 96]
    obs = defaultdict(lambda: None, setting["observation_params"])
    sc = Scenario(T, setting["problem_params"], setting["store_params"], setting["warehouse_params"], setting["echelon_params"], n,
                  obs, setting["seeds"], sampler="hip", device=DEV)
    data = {k: v.to(DEV) for k, v in sc.get_data().items()}
    torch.manual_seed(13)
    model = NeuralNetworkCreator().create_neural_network(sc, policy, device=DEV)
    eng = _engine(model, setting, data, obs, "bf16", use_graph=graph)
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    for step in range(3):
        opt.zero_grad()
        eng.run(data, T, 0, train=True, observation_params=obs)
        torch.cuda.synchronize()
        if step < 2:
            opt.step()   # (the weights move: the next run must refresh its bf16 copies)
    if graph:
        assert set(eng._graphs) == {"fwd", "bwd"}
    lins = model.master_linears()
    assert [(m.out_features, m.in_features) for m in lins[1:4]] == [(160, 256), (288, 160), (96, 288)]
    assert eng.bf16_layers == [1, 2]
    assert eng.dZhist is not None and all(h.shape[0] == T for h in eng.hidden), \
        "the engine did not keep the per-period histories (period-by-period weight gradients): nothing to check in place"
    nc = (n + 3) // 4 * 4
    grads = {id(p): g for p, g in eng.param_grads()}
    worst = defaultdict(float)
    for i in eng.bf16_layers:
        W, bias = lins[i].weight.detach(), lins[i].bias.detach()
        N, K = W.shape
        # the copies the kernels read: the bf16 rounding of the weights as the optimizer left them
        assert torch.equal(eng.Wb[i][:, :K], W.to(torch.bfloat16)), f"layer {i}: stale or wrong Wb"
        assert torch.equal(eng.Wtb[i][:, :N], W.t().to(torch.bfloat16)), f"layer {i}: stale or wrong Wtb"
        for t in range(T):
            x, y = eng.hidden[i - 1][t], eng.hidden[i][t]
            ref, tol = emu.forward(W, x[:, :nc], bias)
            worst["forward"] = max(worst["forward"], _within(y[:, :nc], ref, tol, f"layer {i}, period {t}: forward"))
            ref, tol = emu.dgrad(W.t(), eng.dZhist[i][t][:, :nc], x[:, :nc])
            worst["dgrad"] = max(worst["dgrad"], _within(eng.dZhist[i - 1][t][:, :nc], ref, tol, f"layer {i}, period {t}: dgrad"))
        # weight and bias gradient: the contraction over all periods (the gradient scale is inside dZhist: g_reward carries it, the
        # slab reduction multiplies by 1)
        ref, tol, ref_b, tol_b = emu.wgrad_periods(eng.dZhist[i][:, :, :n], eng.hidden[i - 1][:, :, :n])
        worst["wgrad"] = max(worst["wgrad"], _within(grads[id(lins[i].weight)], ref, tol, f"layer {i}: weight gradient"),
                             _within(grads[id(lins[i].bias)], ref_b, tol_b, f"layer {i}: bias gradient"))
    # the ineligible layer 3 is the FP32 engine's arithmetic, bit for bit: bf16 mode changes nothing outside bf16_layers
    assert 3 not in eng.Wb and 3 not in eng.Wtb
    for t in range(T):
        y = torch.full_like(eng.hidden[3][t], NAN)
        ops.linear_fwd(eng.Wp[3][:, :288], lins[3].bias.detach(), eng.hidden[2][t], y, n, _lib.NIC_ACT_ELU)
        assert torch.equal(y[:, :nc], eng.hidden[3][t][:, :nc]), f"layer 3, period {t}: not the FP32 kernel's output"
    print(f"RATIO engine in place ({'graph replay' if graph else 'eager'}, {n} x T={T}, tail={eng._use_tail()}): "
          + ", ".join(f"{k} {v:.4f}" for k, v in worst.items()))
