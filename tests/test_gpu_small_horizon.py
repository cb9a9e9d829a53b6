"""`nic_small_rollout_fwd / _bwd_wgrad / _bwd / _reduce` (csrc/small_rollout.hip, small_rollout16.hip) through the C ABI against the
float64 rollout of tests/small_horizon_cases.py, row by row: every single-model instantiation by name at both lane widths, the
width-32 histories, the dz rows, every packed parameter gradient, what lies outside the written region, and what the launchers
refuse.  The bar is measured against the reference's own float32 run (small_horizon_cases.bar)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import small_horizon_cases as sc  # noqa: E402
from neural_inventory_control_amd import _lib  # noqa: E402
from neural_inventory_control_amd import small_rollout as sr  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0) if torch.cuda.is_available() else None
NAN = float("nan")
HIST = ("states_hist", "hidden_hist", "logits_hist")
RATIOS = {}   # (recorded kernel name, quantity) -> (worst e_kernel / e32 of this session, case)


def _last_kernel():
    return _lib.lib().nic_last_kernel().decode()


def _bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _forward(L, with_hist):
    h = [b.buf for b in L.hist] if with_hist else [None] * 3
    sr.small_rollout_fwd(L.desc, L.rewards.buf, L.state_final.buf, *h)
    torch.cuda.synchronize()
    return _last_kernel()


def _check_totals(L):
    """nic_small_rollout_reduce on the costs, padding columns (the caller's zeros) included, against their float64 sums.  Bound:
    every lane adds ceil(n / 4 / 256) float4 sums serially, then an 8-level tree, twice (two stages): (n / 1024 + 24) roundings of
    2^-24 relative to sum|x|."""
    c = L.case
    costs = L.rewards.view()[0]   # [T][ldb]
    n = costs.numel()
    scratch = torch.full((sr.small_rollout_reduce_scratch(0, 0, n),), NAN, device=DEV)
    for ignore in (0, 1):
        totals = torch.full((2,), NAN, device=DEV)
        sr.small_rollout_reduce(None, 0, None, costs, ignore, totals, scratch)
        torch.cuda.synchronize()
        want = torch.stack([costs.double().sum(), costs[ignore:].double().sum()]).cpu()
        bound = (n / 1024 + 24) * 2.0 ** -24 * float(costs.double().abs().sum())
        err = (totals.cpu().double() - want).abs()
        print(f"{c.id:16s} totals ignore_periods {ignore}: {totals.tolist()}  float64 {want.tolist()}  |diff| {err.tolist()}  bound {bound:.2e}")
        assert bool((err <= bound).all()), (c.id, ignore, err.tolist(), bound)


def _note(name, ratios, quantities, cid):
    for q in quantities:
        if q in ratios and ratios[q] >= RATIOS.get((name, q), (-1.0, None))[0]:
            RATIOS[name, q] = (ratios[q], cid)


@pytest.mark.parametrize("width", [32, 16])
@pytest.mark.parametrize("c", sc.SMALL_HORIZON_CASES, ids=sc.CASE_IDS)
def test_small_rollout_kernels_match_float64_rollout(c, width):
    """Every figure is printed before it is asserted (-s)."""
    names = dict(zip(sc.LAUNCHES, sc.EXPECTED_KERNELS[c.id]))
    want_fwd, want_wgrad, want_dz = names[f"fwd{width}"], names[f"wgrad{width}"], names["dz32"] if width == 32 else None
    Fd, n_out, P = sc.dims_of(c)
    L = sc.prepare(c, width, DEV)
    # forward without histories, then with them: the same rewards and final state, bit for bit
    assert _forward(L, with_hist=False) == want_fwd
    plain = (L.rewards.buf.clone(), L.state_final.buf.clone())
    assert L.rewards.outside_untouched(), (c.id, "rewards written outside (t < T, b < B): the padding columns are no longer zero")
    assert L.state_final.outside_untouched()
    assert all(b.untouched() for b in L.hist)
    L.rewards, L.state_final = sc.Buf(1, c.T, c.ldb, c.B, DEV, pad=0.0), sc.Buf(Fd, 1, c.ldb, c.B, DEV)
    assert _forward(L, with_hist=True) == want_fwd
    assert _bits(L.rewards.buf, plain[0]) and _bits(L.state_final.buf, plain[1])
    got = dict(rewards=L.rewards.get()[0], state_final=L.state_final.get()[:, 0])
    assert bool(torch.isfinite(got["rewards"]).all()) and bool(torch.isfinite(got["state_final"]).all())
    if width == 32:   # (the width-16 history order is private to its forward / backward pair: checked through the gradients)
        for n, b in zip(HIST, L.hist):
            assert b.outside_untouched(), (c.id, n, "written outside (row < rows, t < T, b < B)")
            got[n] = b.get()
    else:
        assert all(bool(torch.isnan(b.buf[-b.TAIL:]).all()) for b in L.hist)
    _check_totals(L)
    failures, ratios = sc.check(c, got, f"w{width}")
    _note(want_fwd, ratios, sc.FORWARD_QUANTITIES, c.id)
    if not c.round_orders:
        keep = sc.kept(c)
        print(f"{c.id:16s} gradients compared on {int(keep.sum())} of {c.B} scenarios")
        before = [b.buf.clone() for b in L.hist]
        sr.small_rollout_bwd_wgrad(L.desc, *(b.buf for b in L.hist), L.g_reward, L.slab)
        torch.cuda.synchronize()
        assert _last_kernel() == want_wgrad
        assert sr.small_rollout_bwd_wgrad_slots(c.B) == L.slab_rows
        rows = sr.slab_rows_written(c.B, width)   # one partial gradient per wavefront; the rest of the slab is not this launch's
        assert bool(torch.isfinite(L.slab[:rows, :P]).all()), (c.id, "a wavefront left part of its slab row unwritten")
        assert bool(torch.isnan(L.slab[:rows, P:]).all()) and bool(torch.isnan(L.slab[rows:]).all())
        grads = sc.unpack_grad(c, L.slab[:rows, :P].double().sum(dim=0).cpu())
        f2, r2 = sc.check(c, grads, f"w{width}")
        _note(want_wgrad, r2, sc.param_quantities(c), c.id)
        failures += f2
        if width == 32:
            sr.small_rollout_bwd(L.desc, *(b.buf for b in L.hist), L.g_reward, L.dz_hidden.buf, L.dz_out.buf)
            torch.cuda.synchronize()
            assert _last_kernel() == want_dz
            assert L.dz_hidden.outside_untouched() and L.dz_out.outside_untouched()
            f3, r3 = sc.check(c, dict(dz_hidden=L.dz_hidden.get(), dz_out=L.dz_out.get()), "dz")
            _note(want_dz, r3, sc.DZ_QUANTITIES, c.id)
            failures += f3
        for n, b, was in zip(HIST, L.hist, before):   # the backward sweeps only read them
            assert _bits(b.buf, was), (c.id, n)
    assert not failures, (c.id, width, failures)


def test_report_the_referee_ratios():
    """(pytest -s) the worst e_kernel / e32 per recorded kernel name of this session (recorded in small_horizon_cases.py and DESIGN.md)"""
    worst = {}
    for (name, q), (ratio, cid) in sorted(RATIOS.items()):
        print(f"referee ratio  {name:50s} {q:12s} {ratio:6.2f}  ({cid})")
        if ratio >= worst.get(name, (-1.0,))[0]:
            worst[name] = (ratio, q, cid)
    for name, (ratio, q, cid) in sorted(worst.items()):
        print(f"worst referee ratio  {name:50s} {ratio:6.2f}  ({q}, {cid})")


# ---- what the launchers refuse: host checks, no kernel runs ------------------------------------------------------------------------
def _refused(L, word, entry="fwd", hist=(True, True, True), slab_stride=None):
    """the entry point returns non-zero with `word` in nic_last_error, nic_last_kernel() stays what it was, and every NaN-filled
    output is untouched"""
    lib, p = _lib.lib(), _lib.ptr
    before = _last_kernel()
    h = [p(b.buf) if on else None for b, on in zip(L.hist, hist)]
    if entry == "fwd":
        st = lib.nic_small_rollout_fwd(L.desc, p(L.rewards.buf), p(L.state_final.buf), *h, _lib.current_stream())
    elif entry == "wgrad":
        st = lib.nic_small_rollout_bwd_wgrad(L.desc, *h, L.g_reward.t2(), p(L.slab), slab_stride or L.slab.stride(0), _lib.current_stream())
    else:
        st = lib.nic_small_rollout_bwd(L.desc, *h, L.g_reward.t2(), p(L.dz_hidden.buf), p(L.dz_out.buf), _lib.current_stream())
    msg = lib.nic_last_error().decode()
    torch.cuda.synchronize()
    assert st != 0, (entry, word)
    assert word in msg, (word, msg)
    assert _last_kernel() == before, (word, "a refused request recorded a kernel")
    assert L.rewards.outside_untouched() and bool(torch.isnan(L.rewards.get()).all()), word
    for b in [L.state_final, L.dz_hidden, L.dz_out] + L.hist:
        assert b.untouched(), word
    assert bool(torch.isnan(L.slab).all()), word


def test_small_rollout_launchers_refuse_what_they_do_not_take():
    L = sc.prepare(sc.case("one-store-h2"), 32, DEV)
    assert _forward(L, with_hist=False) == sc.EXPECTED_KERNELS["one-store-h2"][0]   # a name for the refusals to leave alone

    def fresh(id, width=32, **fields):
        L = sc.prepare(sc.case(id), width, DEV)
        for n, v in fields.items():
            setattr(L.desc, n, v)
        return L

    for entry in ("fwd", "wgrad", "dz"):
        _refused(fresh("ws2-min", Ws=1, F=1), "unsupported chain", entry)                       # a one-slot pipeline
        _refused(fresh("ws16", Ws=17, F=17), "F mismatch / too large", entry)
        _refused(fresh("ech3-F16", We=5, F=19), "F mismatch / too large", entry)
        _refused(fresh("ws3", F=4), "F mismatch / too large", entry)                             # F is not the sum of the slots
        _refused(fresh("ech1", F=6), "F mismatch / too large", entry)
        _refused(fresh("ech1", Wn=0, F=4), "echelons need the warehouse", entry)
        _refused(fresh("ws3", n_out=2), "n_out does not match the head", entry)
        _refused(fresh("ech1", n_out=2), "n_out does not match the head", entry)
        _refused(fresh("ws3", n_hidden=0), "n_hidden must be 1..3", entry)
        _refused(fresh("ws3", n_hidden=4), "n_hidden must be 1..3", entry)
        _refused(fresh("ws3", lane_scenarios=8), "lane_scenarios must be 0, 16 or 32", entry)
    for entry in ("fwd", "wgrad"):
        _refused(fresh("one-store-h2", width=16, ldb=40), "multiple of 16", entry)              # (B = 33 <= 40: only the width objects)
    _refused(fresh("ws3", width=16), "dz-history sweep", "dz")
    L = fresh("serial-h2")
    _refused(L, "shorter than the packed weights", "wgrad", slab_stride=L.P - 1)
    for missing in range(3):
        hist = tuple(i != missing for i in range(3))
        _refused(fresh("serial-h2"), "incomplete history buffers", "fwd", hist)
        _refused(fresh("serial-h2"), "null buffer", "wgrad", hist)
        _refused(fresh("serial-h2"), "null buffer", "dz", hist)
    assert _last_kernel() == sc.EXPECTED_KERNELS["one-store-h2"][0]
