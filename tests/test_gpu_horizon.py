"""`nic_horizon_rollout_fwd / _bwd` (csrc/horizon_rollout.hip) through the C ABI against the float64 rollout of tests/horizon_cases.py,
element by element: every instantiation by name, every history, the three pre-activation gradients, what lies outside the live
region, and what the launchers refuse.  The bar is measured against the reference's own float32 run (horizon_cases.bar)."""
import os
import sys
import types

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import horizon_cases as hc  # noqa: E402
from neural_inventory_control_amd import _lib  # noqa: E402
from neural_inventory_control_amd import horizon_rollout as hz  # noqa: E402
from neural_inventory_control_amd._lib import NicHorizonDesc  # noqa: E402
from neural_inventory_control_amd.layout import EnvProblem, Table  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0) if torch.cuda.is_available() else None
_NAN = float("nan")


def _sentinel(*shape):
    return torch.full(shape, _NAN, device=DEV)


class _Hist:
    """A history of `rows` rows in the kernels' layout - element (row, t, b) at row * hist_stride + t * ldb + b - inside a buffer
    that is NaN everywhere else: one spare row, the stride gap, the padding columns."""

    def __init__(self, rows, T, ldb, stride, B, values=None):
        self.rows, self.T, self.ldb, self.B = rows, T, ldb, B
        self.buf = _sentinel(rows + 1, stride)
        if values is not None:
            self.live()[:] = values.to(DEV)

    def live(self):
        return self.buf[:self.rows, :self.T * self.ldb].view(self.rows, self.T, self.ldb)[:, :, :self.B]

    def outside_untouched(self):
        rest = self.buf.clone()
        rest[:self.rows, :self.T * self.ldb].view(self.rows, self.T, self.ldb)[:, :, :self.B] = _NAN
        return torch.equal(rest.view(torch.int32), torch.full_like(rest, _NAN).view(torch.int32))

    def get(self):
        return self.live().cpu().double()


def prepare(c):
    """descriptor + every buffer of one case; inputs carry NaN wherever the kernels must not look (or must not let it through)"""
    k = hc.make_inputs(c)
    FD, n_out, n_ord = hc.dims_of(c)
    B, T, ld, S, Wn = c.B, c.T, c.ldb, c.S, c.Wn
    hs = T * ld + c.hist_gap
    L = types.SimpleNamespace(case=c, hs=hs)
    prob = EnvProblem(k["problem"], {n: v.to(DEV) for n, v in k["data"].items()}, DEV)
    for name in ("underage", "holding", "lead", "wh_holding", "wh_lead", "wh_edge"):   # the case's choice of table layout took
        tab = getattr(prob, name)
        if tab.tensor is not None and B > 1:
            assert (tab.scn_stride == 1) == c.per_scenario, (c.id, name)
    dem = _sentinel(c.t0 + T + 1, S, ld)
    dem[:, :, :B] = k["data"]["demands"].permute(2, 1, 0).to(DEV)
    st = [k["data"]["initial_inventories"].flatten(1)] + ([k["data"]["initial_warehouse_inventories"].flatten(1)] if Wn else [])
    L.state0 = _sentinel(FD, ld)
    L.state0[:, :B] = torch.cat(st, dim=1).t().to(DEV)
    L.mask = k["mask"].to(DEV).contiguous() if Wn else None
    if c.mode == 0:
        L.lin = [types.SimpleNamespace(weight=k[w].to(DEV), bias=None if b is None else k[b].to(DEV))
                 for w, b in (("W1", None), ("W2", "b2"), ("W3", "b3"))]
        d = hz.HorizonPlan(prob, [FD + c.w_gap, c.H1, c.H2, n_out]).desc(prob, T, c.t0, L.lin, L.mask, dem, hs)
        assert (d.ldw1, d.ldw2, d.ldw3) == (FD + c.w_gap, c.H1 + c.w_gap, c.H2 + c.w_gap)
        L.z1_obs = _Hist(c.H1, T, ld, hs, B, k["z1_obs"])
        L.tape = None
    else:   # the plan only describes the policy MLP: a tape descriptor is filled in as TapeRollout fills it
        d = NicHorizonDesc()
        d.io = prob.make_io(None, None, None, Table.null(), Table.null(), None, None)
        d.T, d.t0, d.H1, d.H2, d.n_out = T, c.t0, 0, 0, n_out
        d.mask, d.demand, d.hist_stride = _lib.ptr(L.mask), dem.data_ptr(), hs
        d.head_mode, d.allow_negative = c.mode, c.allow_negative
        L.tape = _Hist(n_ord if c.mode == 1 else S, T, ld, hs, B, k["tape"])
        d.tape = L.tape.buf.data_ptr()
        L.z1_obs = None
    d.io.dims.ldb = ld   # (EnvProblem pads to 64 columns; its tables keep their own strides)
    L.desc, L.keep = d, (prob, dem)
    L.rewards = _Hist(1, T, ld, T * ld, B)
    L.state_final = _Hist(FD, 1, ld, ld, B)
    H = lambda rows: _Hist(rows, T, ld, hs, B)   # noqa: E731
    L.hist = dict(state_hist=H(FD), orders_hist=H(n_ord + Wn))
    if c.mode == 0:
        L.hist.update(h1_hist=H(c.H1), h2_hist=H(c.H2), logits_hist=H(n_out))
    L.dz = {}
    if c.mode == 0:
        L.dz = dict(dz1_hist=H(c.H1), dz2_hist=H(c.H2), dz3_hist=H(n_out))
    elif c.mode == 2:
        L.dz = dict(dz3_hist=H(S))
    g = k["g_reward"]
    if c.g_uniform:
        L.g_reward = Table(g[:1].contiguous().to(DEV), 0, 0)
    else:
        gt = _sentinel(ld)
        gt[:B] = g.to(DEV)
        L.g_reward = Table(gt, 0, 1)
    return L


def _buf(h):
    return None if h is None else h.buf


def forward(L, with_hist):
    h = L.hist if with_hist else {}
    hz.horizon_fwd(L.desc, _buf(L.z1_obs), L.state0, L.rewards.buf, L.state_final.buf, *(
        _buf(h.get(n)) for n in ("state_hist", "h1_hist", "h2_hist", "logits_hist", "orders_hist")))
    torch.cuda.synchronize()
    return _lib.lib().nic_last_kernel().decode()


def backward(L):
    hz.horizon_bwd(L.desc, *(_buf(L.hist.get(n)) for n in ("state_hist", "h1_hist", "h2_hist", "logits_hist", "orders_hist")),
                   L.g_reward, *(_buf(L.dz.get(n)) for n in ("dz1_hist", "dz2_hist", "dz3_hist")))
    torch.cuda.synchronize()
    return _lib.lib().nic_last_kernel().decode()


def _compare(c, got, names, cols, failures, ratios):
    r64, e32 = hc.reference(c, torch.float64), hc.yardstick(c)
    for n in names:
        e, row = hc.row_errors(n, got[n], r64[n], cols)
        zero = hc.zero_rows(n, r64[n], cols)
        g = hc.as_rows(n, got[n])
        g = g if cols is None else g[..., cols]
        ratios[n] = e / e32[n] if e32[n] > 0 else (0.0 if e == 0 else float("inf"))
        print(f"{c.id:15s} {n:12s} e_kernel {e:.2e} (row {row})  e32 {e32[n]:.2e}  ratio {ratios[n]:.2f}  bar {hc.bar(e32[n]):.2e}  "
              f"zero rows {int(zero.sum())}")
        if not bool((g[zero] == 0).all()):
            failures.append((n, "a row that is identically zero in the reference is not exactly zero"))
        if not e <= hc.bar(e32[n]):
            failures.append((n, f"e_kernel {e:.3e} at row {row} above the bar {hc.bar(e32[n]):.3e} (e32 {e32[n]:.3e})"))


@pytest.mark.parametrize("c", hc.ALL_CASES, ids=hc.CASE_IDS)
def test_horizon_kernels_match_float64_rollout(c):
    """Every figure is printed before it is asserted (-s).  Measured on one MI355X, worst e_kernel / e32 per instantiation: forward
    <8,16> 2.21, <8,40> 3.76, <8,64> 7.76; backward <8,0> 1.31, <8,1> 1.48, <8,2> 2.24 (bar 10; horizon_cases.HORIZON_CASES)."""
    want_fwd, want_bwd = hc.expected_kernels(c)
    L = prepare(c)
    assert hz.horizon_ok(L.desc), _lib.lib().nic_last_error()
    failures, ratios = [], {}
    # forward without histories, then with them: the same rewards and final state, bit for bit
    assert forward(L, with_hist=False) == want_fwd
    plain = (L.rewards.get(), L.state_final.get())
    assert L.rewards.outside_untouched() and L.state_final.outside_untouched()
    assert all(h.outside_untouched() and bool(torch.isnan(h.get()).all()) for h in L.hist.values())
    L.rewards.buf.fill_(_NAN)
    L.state_final.buf.fill_(_NAN)
    assert forward(L, with_hist=True) == want_fwd
    got = dict(rewards=L.rewards.get()[0], state_final=L.state_final.get()[:, 0], **{n: h.get() for n, h in L.hist.items()})
    assert torch.equal(got["rewards"], plain[0][0]) and torch.equal(got["state_final"], plain[1][:, 0])
    for n, h in dict(L.hist, rewards=L.rewards, state_final=L.state_final).items():
        assert h.outside_untouched(), (c.id, n, "written outside (row < rows, t < T, b < B)")
    _compare(c, got, [n for n in hc.FORWARD_QUANTITIES if n in got], None, failures, ratios)
    if c.mode != 1:
        keep = hc.kept(c)
        print(f"{c.id:15s} gradients compared on {int(keep.sum())} of {c.B} scenarios ({c.B - int(keep.sum())} knife edges excluded)")
        assert backward(L) == want_bwd
        for n, h in L.dz.items():
            assert h.outside_untouched(), (c.id, n, "written outside (row < rows, t < T, b < B)")
        for n, h in L.hist.items():   # the backward only reads them
            assert torch.equal(h.get(), got[n]), (c.id, n)
        _compare(c, {n: h.get() for n, h in L.dz.items()}, list(L.dz), keep, failures, ratios)
    print(f"{c.id:15s} {want_fwd} / {want_bwd if c.mode != 1 else '-'}: worst ratio forward "
          f"{max(ratios[n] for n in ratios if n in hc.FORWARD_QUANTITIES):.2f}, backward "
          f"{max([ratios[n] for n in ratios if n in hc.GRAD_QUANTITIES], default=0.0):.2f}")
    assert not failures, (c.id, failures)


def _refused(d, word):
    """nic_horizon_rollout_ok says no, and the launcher returns a status whose message names the limit.  Every data pointer of the
    launch itself is NULL: had the descriptor passed, the launcher would stop at its null checks - nothing reaches the device."""
    lib = _lib.lib()
    assert lib.nic_horizon_rollout_ok(d) == 0, word
    st = lib.nic_horizon_rollout_fwd(d, None, None, None, None, None, None, None, None, None, None)
    assert st != 0, word
    msg = lib.nic_last_error().decode()
    assert word in msg, (word, msg)


def _case(id):
    return next(c for c in hc.ALL_CASES if c.id == id)


def test_horizon_launchers_refuse_what_they_do_not_take():
    lib = _lib.lib()
    for c in hc.ALL_CASES:
        assert lib.nic_horizon_rollout_ok(prepare(c).desc) == 1, (c.id, lib.nic_last_error())

    def variant(id, **dims):
        L = prepare(_case(id))
        for n, v in dims.items():
            setattr(L.desc.io.dims, n, v)
        D = L.desc.io.dims
        L.desc.n_out = D.n_warehouses + D.n_stores * D.n_warehouses if D.n_warehouses else D.n_stores
        return L

    L = variant("S64-Wn0", n_stores=65, store_slots=2)
    _refused(L.desc, "1..64 stores")
    L = variant("Wn32", n_stores=1, n_warehouses=33)
    _refused(L.desc, "at most 32 warehouses")
    for slots in (1, 9):
        L = variant("stores-only", store_slots=slots)
        _refused(L.desc, "pipelines of 2..8 slots")
        L = variant("nout16", store_slots=2, warehouse_slots=slots)
        _refused(L.desc, "pipelines of 2..8 slots")
    L = variant("FD65", n_stores=51, store_slots=5, n_warehouses=1, warehouse_slots=2)
    _refused(L.desc, "257 state rows")
    L = variant("ref", n_stores=42, store_slots=2, n_warehouses=3, warehouse_slots=2)
    _refused(L.desc, "129 logits rows")
    for field in ("H1", "H2"):
        L = prepare(_case("ref"))
        setattr(L.desc, field, 65)
        _refused(L.desc, "hidden widths 1..64")
    L = variant("ref", ldb=56)
    _refused(L.desc, "bad n_scenarios / ldb")
    L = prepare(_case("ref"))
    L.desc.hist_stride = L.case.T * L.case.ldb - 1
    _refused(L.desc, "hist_stride")
    L = variant("ref", n_echelons=1)
    _refused(L.desc, "extra echelons")
    L = prepare(_case("orders-S7"))   # an order tape with two warehouses, read as levels
    L.desc.head_mode = 2
    _refused(L.desc, "no warehouses")
    # backward: refused for an order tape and under round_orders (the forward takes both)
    L = prepare(_case("orders-S7"))
    assert lib.nic_horizon_rollout_ok(L.desc) == 1
    st = lib.nic_horizon_rollout_bwd(L.desc, None, None, None, None, None, Table.null().t2(), None, None, None, None)
    assert st != 0 and "order tape has no gradient" in lib.nic_last_error().decode()
    L = prepare(_case("min"))   # (real buffers of a valid case: this check comes after the launcher's null checks)
    L.desc.round_orders = 1
    p = _lib.ptr
    st = lib.nic_horizon_rollout_bwd(L.desc, *(p(L.hist[n].buf) for n in ("state_hist", "h1_hist", "h2_hist", "logits_hist", "orders_hist")),
                                     L.g_reward.t2(), *(p(L.dz[n].buf) for n in ("dz1_hist", "dz2_hist", "dz3_hist")), None)
    assert st != 0 and "rounded orders have no gradient" in lib.nic_last_error().decode()
    assert bool(torch.isnan(L.dz["dz3_hist"].buf).all())
