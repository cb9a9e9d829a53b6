"""The small-policy whole-horizon kernels (csrc/small_rollout.hip, small_rollout16.hip, small_rollout_mfma.h) against a plain torch
rollout in float64: case table, inputs, reference, a float32 emulation with switchable defects, and the checker.

No GPU is needed here (torch, the oracle's env step, ctypes descriptors).  tests/test_small_horizon_cases_host.py asserts the
conditions on the inputs from the reference alone, shows that the checker fails under each planted defect, and runs the host build
of small_rollout_body.h through it; tests/test_gpu_small_horizon.py launches `nic_small_rollout_fwd / _bwd_wgrad / _bwd / _reduce`
through the C ABI on the same table.

The reference rolls T periods of `Trainer.simulate_batch` for one store (optionally behind a warehouse and E echelons):
    x = [store slots | warehouse slots | echelon slots]  (detached when `detach`);  h_l = ELU(W_l h_{l-1} + b_l), 32 wide;  z = Wout h + bout
    head 0 (vanilla_one_store): order = softplus(z + 1)
    head 1 (vanilla_serial):    rows [echelons..., warehouse, store] = sigmoid(z) * [upper_bound, echelon on-hands..., warehouse on-hand]
    oracle.env_step
with loss = sum_t sum_b g_reward[b] * reward[t, b].  Parameter gradients are autograd's, in the packed-weight layout; the
pre-activation gradients are those of zero-valued probes added to every layer's pre-activation.

Bar: per quantity, row by row, e(row) = max|x - ref64| / max|ref64 row|; a quantity passes when its worst row has
e_kernel <= max(10 * worst-row e32, 2e-6), e32 being the float32 run of this very reference (never the kernel).  A parameter
gradient tensor is one row.  Gradients are compared on the scenarios whose smallest decision margin exceeds 1e-4 (`KNIFE_EDGE`):
the pre-activation gradients on those columns, the parameter gradients with g_reward set to zero on the others, in the reference
and in the launch alike.  Forward quantities are compared on all scenarios (under `round_orders` on those whose orders all stay
further than the margin from a half-integer: a rounded order is not continuous).
"""
import functools
import types
from collections import namedtuple

import torch
import torch.nn.functional as F

from neural_inventory_control_amd import small_rollout as sr
from neural_inventory_control_amd.layout import EnvProblem, Table
from oracle import inventory_oracle as orc

KNIFE_EDGE = 1e-4        # as tests/horizon_cases.py
MAX_EXCLUDED = 0.25      # at most a quarter of a case's scenarios may be knife edges
BAR_FACTOR, BAR_FLOOR = 10.0, 2e-6
H = 32
NAN = float("nan")

SCase = namedtuple("SCase", "id seed head Ws Ww E We n_hidden B T t0 profit lost edge per_scenario g_uniform ldb detach round_orders "
                            "demand_extra")


def C(id, seed, head, Ws, n_hidden, B, T, Ww=0, E=0, We=0, t0=0, profit=False, lost=True, edge=False, per_scenario=False,
      g_uniform=False, ldb=None, detach=None, round_orders=0, demand_extra=1):
    ldb = ldb or -(-B // 16) * 16
    assert ldb % 16 == 0 and ldb >= B and (head == 1 or (Ww, E, We) == (0, 0, 0)) and (head == 0 or Ww >= 2) and (E == 0 or We >= 2)
    detach = head if detach is None else detach   # (the engines' default: vanilla_serial's MLP input carries no gradient)
    return SCase(id, seed, head, Ws, Ww, E, We, n_hidden, B, T, t0, profit, lost, edge and head == 1, per_scenario, g_uniform, ldb, detach,
                 round_orders, demand_extra)


# The smallest shapes at which each thing can go wrong: every (route, chain shape, n_hidden) cell of sr_variant at both lane widths,
# the chains at the limits the launcher admits, ragged and full wavefronts (B 1 .. 65), T 1 / 2 / longer than the pipeline + 1, t0 2.
# (measured ratios: below the table of expected names)
SMALL_HORIZON_CASES = [
    # head 0: one store
    C("ws2-min", 101, 0, 2, 1, B=1, T=6, g_uniform=True),                                 # the shortest pipeline, T > Ws + 1, one scenario
    C("ws16", 102, 0, 16, 2, B=15, T=3, lost=False, per_scenario=True),                   # F = 16 in one pipeline
    C("ws3", 203, 0, 3, 3, B=17, T=5, t0=2, profit=True, per_scenario=True, ldb=32, demand_extra=3),
    C("ws3-detach", 104, 0, 3, 2, B=31, T=5, detach=1, lost=False, ldb=32),               # detach_input on the softplus head
    C("one-store-h1", 105, 0, 4, 1, B=16, T=1, g_uniform=True),                           # one full 16-block, one period: every gradient is an exact zero
    C("one-store-h2", 106, 0, 4, 2, B=33, T=2, per_scenario=True, ldb=80),                # ldb > pad_ld(B) = 64, three 16-blocks
    C("one-store-h3", 107, 0, 4, 3, B=65, T=6, t0=2, lost=False, profit=True, ldb=80, demand_extra=2),
    C("one-store-round", 108, 0, 4, 3, B=40, T=5, per_scenario=True, ldb=48, round_orders=1),   # forward only
    # head 1: store + warehouse (+ echelons)
    C("wh-only", 111, 1, 3, 2, B=32, T=4, Ww=2, per_scenario=True, edge=True),            # Wn = 1, E = 0: n_out = 2
    C("ech1", 112, 1, 2, 1, B=17, T=5, Ww=3, E=1, We=2, t0=2, detach=0, lost=False, ldb=32, demand_extra=2),
    C("ech3-F16", 113, 1, 2, 3, B=40, T=4, Ww=2, E=3, We=4, per_scenario=True, edge=True, ldb=48),   # F = 2 + 2 + 3 * 4, n_out = 5
    C("serial-h1", 114, 1, 4, 1, B=15, T=1, Ww=3, E=2, We=4, g_uniform=True, profit=True),
    C("serial-h2", 115, 1, 4, 2, B=33, T=6, Ww=3, E=2, We=4, t0=2, per_scenario=True, ldb=48, demand_extra=2),
    C("serial-h3", 116, 1, 4, 3, B=16, T=2, Ww=3, E=2, We=4, detach=0, lost=False, edge=True, per_scenario=True),
]
CASE_IDS = [c.id for c in SMALL_HORIZON_CASES]
assert len(set(CASE_IDS)) == len(CASE_IDS)

# what nic_last_kernel() reports after each launch of a case: forward and in-kernel-wgrad backward at 32 scenarios per wavefront,
# the dz-history backward (32 only), forward and backward at 16.  (The recorded name states the request - csrc/small_rollout_variants.h.)
EXPECTED_KERNELS = {
    "ws2-min": ("small_rollout_fwd_mfma_kernel<1,any>", "small_rollout_bwd_mfma_kernel<1,wgrad,any>", "small_rollout_bwd_mfma_kernel<1,any>",
                "small_rollout16_fwd_kernel<1,any>", "small_rollout16_bwd_kernel<1,wgrad,any>"),
    "ws16": ("small_rollout_fwd_mfma_kernel<2,any>", "small_rollout_bwd_mfma_kernel<2,wgrad,any>", "small_rollout_bwd_mfma_kernel<2,any>",
             "small_rollout16_fwd_kernel<2,any>", "small_rollout16_bwd_kernel<2,wgrad,any>"),
    "ws3": ("small_rollout_fwd_mfma_kernel<3,any>", "small_rollout_bwd_mfma_kernel<3,wgrad,any>", "small_rollout_bwd_mfma_kernel<3,any>",
            "small_rollout16_fwd_kernel<3,any>", "small_rollout16_bwd_kernel<3,wgrad,any>"),
    "ws3-detach": ("small_rollout_fwd_mfma_kernel<2,any>", "small_rollout_bwd_mfma_kernel<2,wgrad,any>", "small_rollout_bwd_mfma_kernel<2,any>",
                   "small_rollout16_fwd_kernel<2,any>", "small_rollout16_bwd_kernel<2,wgrad,any>"),
    "one-store-h1": ("small_rollout_fwd_mfma_kernel<1,one_store>", "small_rollout_bwd_mfma_kernel<1,wgrad,one_store>",
                     "small_rollout_bwd_mfma_kernel<1,one_store>", "small_rollout16_fwd_kernel<1,one_store>",
                     "small_rollout16_bwd_kernel<1,wgrad,one_store>"),
    "one-store-h2": ("small_rollout_fwd_mfma_kernel<2,one_store>", "small_rollout_bwd_mfma_kernel<2,wgrad,one_store>",
                     "small_rollout_bwd_mfma_kernel<2,one_store>", "small_rollout16_fwd_kernel<2,one_store>",
                     "small_rollout16_bwd_kernel<2,wgrad,one_store>"),
    "one-store-h3": ("small_rollout_fwd_mfma_kernel<3,one_store>", "small_rollout_bwd_mfma_kernel<3,wgrad,one_store>",
                     "small_rollout_bwd_mfma_kernel<3,one_store>", "small_rollout16_fwd_kernel<3,one_store>",
                     "small_rollout16_bwd_kernel<3,wgrad,one_store>"),
    "one-store-round": ("small_rollout_fwd_mfma_kernel<3,one_store>", None, None, "small_rollout16_fwd_kernel<3,one_store>", None),
    "wh-only": ("small_rollout_fwd_mfma_kernel<2,any>", "small_rollout_bwd_mfma_kernel<2,wgrad,any>", "small_rollout_bwd_mfma_kernel<2,any>",
                "small_rollout16_fwd_kernel<2,any>", "small_rollout16_bwd_kernel<2,wgrad,any>"),
    "ech1": ("small_rollout_fwd_mfma_kernel<1,any>", "small_rollout_bwd_mfma_kernel<1,wgrad,any>", "small_rollout_bwd_mfma_kernel<1,any>",
             "small_rollout16_fwd_kernel<1,any>", "small_rollout16_bwd_kernel<1,wgrad,any>"),
    "ech3-F16": ("small_rollout_fwd_mfma_kernel<3,any>", "small_rollout_bwd_mfma_kernel<3,wgrad,any>", "small_rollout_bwd_mfma_kernel<3,any>",
                 "small_rollout16_fwd_kernel<3,any>", "small_rollout16_bwd_kernel<3,wgrad,any>"),
    "serial-h1": ("small_rollout_fwd_mfma_kernel<1,serial>", "small_rollout_bwd_mfma_kernel<1,wgrad,serial>",
                  "small_rollout_bwd_mfma_kernel<1,serial>", "small_rollout16_fwd_kernel<1,serial>", "small_rollout16_bwd_kernel<1,wgrad,serial>"),
    "serial-h2": ("small_rollout_fwd_mfma_kernel<2,serial>", "small_rollout_bwd_mfma_kernel<2,wgrad,serial>",
                  "small_rollout_bwd_mfma_kernel<2,serial>", "small_rollout16_fwd_kernel<2,serial>", "small_rollout16_bwd_kernel<2,wgrad,serial>"),
    "serial-h3": ("small_rollout_fwd_mfma_kernel<3,serial>", "small_rollout_bwd_mfma_kernel<3,wgrad,serial>",
                  "small_rollout_bwd_mfma_kernel<3,serial>", "small_rollout16_fwd_kernel<3,serial>", "small_rollout16_bwd_kernel<3,wgrad,serial>"),
}
LAUNCHES = ("fwd32", "wgrad32", "dz32", "fwd16", "wgrad16")
assert set(EXPECTED_KERNELS) == set(CASE_IDS)

# Measured on one MI355X (tests/test_gpu_small_horizon.py::test_report_the_referee_ratios), worst e_kernel / e32 over the cases and
# quantities per recorded name <n_hidden,chain> (the factor of the bar is 10; below e32 = 2e-7 the floor of 2e-6 decides):
#   small_rollout_fwd_mfma_kernel   <1,any> 3.34  <2,any> 2.93  <3,any> 2.95  <1,one_store> 5.57  <2,one_store> 2.79  <3,one_store> 1.65
#                                   <1,serial> 1.33  <2,serial> 1.42  <3,serial> 1.36
#   small_rollout16_fwd_kernel      <1,any> 5.93  <2,any> 3.74  <3,any> 4.28  <1,one_store> 3.37  <2,one_store> 2.61  <3,one_store> 1.21
#                                   <1,serial> 1.44  <2,serial> 1.00  <3,serial> 1.00
#   small_rollout_bwd_mfma_kernel   (dz) <1,any> 1.94  <2,any> 4.43  <3,any> 1.32  <2,one_store> 1.01  <3,one_store> 1.12
#                                   <1,serial> 1.51  <2,serial> 1.60  <3,serial> 1.33;  <1,one_store>: exact zeros (T = 1)
#   small_rollout_bwd_mfma_kernel   (wgrad) <1,any> 2.53  <2,any> 2.49  <3,any> 22.15 (g_b3 of ws3: e32 1.0e-8, a sixth of a rounding;
#                                   e_kernel 2.3e-7 against the floor)  <2,one_store> 2.20  <3,one_store> 1.86  <1,serial> 1.00
#                                   <2,serial> 3.57  <3,serial> 6.03
#   small_rollout16_bwd_kernel      (wgrad) <1,any> 3.60  <2,any> 2.62  <3,any> 16.86 (the same row)  <2,one_store> 2.60
#                                   <3,one_store> 1.21  <1,serial> 3.49  <2,serial> 2.22  <3,serial> 6.03
# Planted defects and the cases they turn red: DESIGN.md, "Small-policy whole-horizon kernels against a float64 rollout".


def dims_of(c):
    """(F, n_out, packed-weight count)"""
    Fd = c.Ws + c.Ww + c.E * c.We
    n_out = 1 if c.head == 0 else c.E + 2
    return Fd, n_out, sr.packed_weight_count(Fd, c.n_hidden, n_out)


def segments(c):
    """[(offset, slots)] of the store, warehouse and echelon pipelines in the state rows"""
    seg = [(0, c.Ws)]
    if c.head == 1:
        seg.append((c.Ws, c.Ww))
        seg += [(c.Ws + c.Ww + e * c.We, c.We) for e in range(c.E)]
    return seg


def case(id):
    return next(c for c in SMALL_HORIZON_CASES if c.id == id)


def _uniform(gen, shape, lo, hi):
    return lo + (hi - lo) * torch.rand(shape, generator=gen)


def _table(gen, B, shape, lo, hi, per_scenario, integer=False):
    """(B, *shape) static table: per scenario, or one row behind an `expand` view (stride 0) as the reference's"""
    n = B if per_scenario else 1
    t = torch.randint(int(lo), int(hi) + 1, (n,) + shape, generator=gen).float() if integer else _uniform(gen, (n,) + shape, lo, hi)
    return t if per_scenario else t.expand((B,) + shape)


UPPER_BOUND = 9.0


@functools.lru_cache(maxsize=None)
def make_inputs(c):
    """Everything a launch reads, float32 on the CPU, in the reference's logical shapes.  Continuous draws, no planted ties: the
    knife edges are measured and excluded, not constructed.  Demand is 0.5 .. 6 a period against 0 .. 4 on hand at the store, so the
    first period already has scenarios on both sides of lost / backlogged demand; upstream slots start at 0.5 .. 5 (positive: the
    serial head orders a share of the on-hand stock, which then stays positive), on both sides of a period's demand.  First-layer
    columns are scaled by the inverse of their state row's typical magnitude."""
    gen = torch.Generator().manual_seed(c.seed)
    B, T, ps = c.B, c.T, c.per_scenario
    Fd, n_out, _ = dims_of(c)
    problem = {"n_stores": 1, "n_warehouses": int(c.head == 1), "n_extra_echelons": c.E, "lost_demand": c.lost, "maximize_profit": c.profit}
    data = {"demands": _uniform(gen, (B, 1, c.t0 + T + c.demand_extra), 0.5, 6.0), "underage_costs": _table(gen, B, (1,), 2.0, 9.0, ps),
            "holding_costs": _table(gen, B, (1,), 0.2, 2.0, ps), "initial_inventories": _uniform(gen, (B, 1, c.Ws), 0.0, 4.0),
            "lead_times": _table(gen, B, (1, 1), 1, c.Ws, ps, integer=True)}
    typ = torch.full((Fd,), 2.0)
    if c.head == 1:
        data["initial_warehouse_inventories"] = _uniform(gen, (B, 1, c.Ww), 0.5, 5.0)
        data["warehouse_holding_costs"] = _table(gen, B, (1,), 0.1, 1.0, ps)
        data["warehouse_lead_times"] = _table(gen, B, (1,), 1, c.Ww, ps, integer=True)
        if c.edge:
            data["warehouse_edge_costs"] = _table(gen, B, (1,), 0.1, 1.0, ps)
        typ[c.Ws:] = 3.0
    if c.E:
        data["initial_echelon_inventories"] = _uniform(gen, (B, c.E, c.We), 0.5, 5.0)
        data["echelon_holding_costs"] = _table(gen, B, (c.E,), 0.05, 0.6, ps)
        data["echelon_lead_times"] = _table(gen, B, (c.E,), 1, c.We, ps, integer=True)
    layers, k = [], Fd
    for i in range(c.n_hidden + 1):
        n = H if i < c.n_hidden else n_out
        W = torch.randn(n, k, generator=gen) * ((1.0 if i < c.n_hidden else 1.5) / k ** 0.5)
        if i == 0:
            W = W / typ[None]
        b = torch.randn(n, generator=gen) * (0.3 if i < c.n_hidden else 0.5)
        if i == c.n_hidden and c.head == 0:
            b = b + 2.0   # softplus(z + 1) around a period's demand
        layers.append((W.contiguous(), b))
        k = n
    n_g = 1 if c.g_uniform else B
    g = _uniform(gen, (n_g,), 0.2, 1.2) * (1 - 2 * (torch.rand(n_g, generator=gen) < 0.3).float())
    return dict(case=c, problem=problem, data=data, layers=layers, g_reward=g.expand(B) if c.g_uniform else g)


_OBS = {"include_static_features": {"holding_costs": True, "underage_costs": True, "lead_times": True},
        "include_days_to_christmas": False, "time_features": None, "sample_features": None}
FORWARD_QUANTITIES = ("rewards", "state_final", "states_hist", "hidden_hist", "logits_hist")
DZ_QUANTITIES = ("dz_hidden", "dz_out")


def param_quantities(c):
    """names of the packed parameter gradients, in packing order: g_w0, g_b0, g_w1, ..."""
    return tuple(f"g_{p}{i}" for i in range(c.n_hidden + 1) for p in "wb")


def unpack_grad(c, packed):
    """packed-weight-layout gradient [P] -> {g_w0: ..., g_b0: ...} (float64)"""
    Fd, n_out, P = dims_of(c)
    assert packed.numel() == P
    out = {}
    for i, (off, n, k, boff) in enumerate(sr.layer_slices(Fd, c.n_hidden, n_out)):
        out[f"g_w{i}"] = packed[off:off + n * k].double().clone()
        out[f"g_b{i}"] = packed[boff:boff + n].double().clone()
    return out


def _rows(x):
    return x.detach().t()


def _note(margins, kind, m, B):
    if m.numel():
        m = m.detach().double().reshape(B, -1).min(dim=1).values
        margins[kind] = torch.minimum(margins[kind], m) if kind in margins else m


def _finish(c, hist, final, loss, params, probes, margins, stats, round_margin):
    """the result dict both rollouts return: float64 tensors in the kernels' layouts"""
    res = {n: torch.stack(hist[n], dim=1).double() for n in ("states_hist", "hidden_hist", "logits_hist")}
    res["rewards"] = torch.stack(hist["rewards"], dim=0).double()
    res["state_final"] = _rows(final).double()
    if not c.round_orders:
        if loss.requires_grad:   # (not for one store and T = 1: the only order is placed after the only cost)
            loss.backward()
        grad = lambda x: (x.grad if x.grad is not None else torch.zeros_like(x)).double()   # noqa: E731
        res["dz_hidden"] = torch.cat([grad(p) for p in probes[:-1]], dim=0)
        res["dz_out"] = grad(probes[-1])
        res.update(unpack_grad(c, torch.cat([grad(t).reshape(-1) for wb in params for t in wb])))
    for v in res.values():
        assert v.dtype == torch.float64
    if margins is not None:
        res["margin"] = torch.stack(list(margins.values())).min(dim=0).values
        res["margins"], res["stats"], res["round_margin"] = margins, stats, round_margin
    return res


@functools.lru_cache(maxsize=None)
def reference(c, dtype):
    """The rollout of case `c` in `dtype` (torch.float64: the referee; torch.float32: the yardstick of the bar) on the oracle's env
    step.  Histories (rows, T, B), rewards (T, B), state_final (F, B), dz rows, the packed parameter gradients by name, plus - per
    scenario - the smallest decision margin and the event counts the host test asserts.  Computed once, never modified.  The loss
    weights g_reward are zero on the scenarios the FLOAT64 run finds on a knife edge, in both runs."""
    k = make_inputs(c)
    B, T = c.B, c.T
    Fd, n_out, _ = dims_of(c)
    f = lambda x: x.to(dtype)   # noqa: E731
    data = {n: f(v) for n, v in k["data"].items()}
    env = orc.env_reset(T, k["problem"], data, dict(_OBS, demand={"past_periods": 0, "period_shift": c.t0},
                                                     include_warehouse_inventory=c.head == 1))
    env.zero_lead_orders = "drop"
    g_reward = f(k["g_reward"]) * (1.0 if dtype == torch.float64 else f(kept(c).double()))
    params = [(W.to(dtype).clone().requires_grad_(True), b.to(dtype).clone().requires_grad_(True)) for W, b in k["layers"]]
    probes = [torch.zeros(W.shape[0], T, B, dtype=dtype, requires_grad=True) for W, _ in params]
    hist = {n: [] for n in ("states_hist", "hidden_hist", "logits_hist", "rewards")}
    margins, round_margin = {}, torch.full((B,), float("inf"), dtype=torch.float64)
    stats = dict(short=0, over=0, bind=0, free=0, arrive=int((k["data"]["lead_times"].reshape(B) <= T - 1).sum()))
    rewards = []
    for t in range(T):
        st = env.obs["store_inventories"]
        parts = [st.flatten(1)]
        if c.head == 1:
            wh = env.obs["warehouse_inventories"]
            parts.append(wh.flatten(1))
        if c.E:
            ech = env.obs["echelon_inventories"]
            parts.append(ech.flatten(1))
        x = torch.cat(parts, dim=1)   # (B, F)
        hist["states_hist"].append(_rows(x))
        h, hid = (x.detach() if c.detach else x), []
        for i, (W, b) in enumerate(params[:-1]):
            h = F.elu(h @ W.t() + b + probes[i][:, t].t())
            hid.append(_rows(h))
        z = h @ params[-1][0].t() + params[-1][1] + probes[-1][:, t].t()
        hist["hidden_hist"].append(torch.cat(hid, dim=0))
        hist["logits_hist"].append(_rows(z))
        d = data["demands"][:, 0, c.t0 + t]
        on_hand = st[:, 0, 0]
        _note(margins, "store", (on_hand - d).abs() / (1 + d), B)
        stats["short"] += int((on_hand < d).sum())
        stats["over"] += int((on_hand > d).sum())
        if c.head == 0:
            orders = F.softplus(z + 1)   # (B, 1)
            up = None
        else:
            up = torch.cat([torch.full((B, 1), UPPER_BOUND, dtype=dtype)] + ([ech[:, :, 0]] if c.E else []) + [wh[:, :, 0]], dim=1)
            orders = torch.sigmoid(z) * up   # rows [echelons..., warehouse, store]
            _note(margins, "order", orders.abs() / (1 + up.abs()), B)
            # what each upstream location keeps after it ships: relu'(.) of its holding cost
            _note(margins, "upstream", (up[:, 1:] - orders[:, 1:]).abs() / (1 + up[:, 1:].abs()), B)
            # the serial head's constraint binds where the warehouse holds less than the period's demand: whatever the logit,
            # the store's order cannot cover it
            stats["bind"] += int((wh[:, 0, 0] < d).sum())
            stats["free"] += int((wh[:, 0, 0] > d).sum())
        if c.round_orders:
            a = orders.detach().double()
            round_margin = torch.minimum(round_margin, ((a - torch.floor(a)) - 0.5).abs().min(dim=1).values)
            orders = torch.round(orders)   # half to even
        action = {"stores": orders[:, -1:].unsqueeze(2)}
        if c.head == 1:
            action["warehouses"] = orders[:, c.E:c.E + 1].unsqueeze(2)
        if c.E:
            action["echelons"] = orders[:, :c.E].unsqueeze(2)
        reward = orc.env_step(env, action)
        hist["rewards"].append(reward.detach())
        rewards.append((g_reward * reward).sum())
    final = torch.cat([env.obs["store_inventories"].flatten(1)] + ([env.obs["warehouse_inventories"].flatten(1)] if c.head == 1 else [])
                      + ([env.obs["echelon_inventories"].flatten(1)] if c.E else []), dim=1)
    return _finish(c, hist, final, sum(rewards), params, probes, margins, stats, round_margin)


def kept(c):
    """scenarios whose gradients are compared: every decision of the float64 run clears the knife-edge threshold"""
    return reference(c, torch.float64)["margin"] > KNIFE_EDGE


def forward_cols(c):
    """columns the forward quantities are compared on: all, or (round_orders) those no order of which is near a half-integer"""
    return reference(c, torch.float64)["round_margin"] > KNIFE_EDGE if c.round_orders else None


def effective_g_reward(c):
    """what a launch passes as g_reward: zero on the knife-edge scenarios (float32, (B,))"""
    return make_inputs(c)["g_reward"] * kept(c).float()


# ---- a float32 emulation with switchable defects: shows that the checker can fail ---------------------------------------------------
DEFECTS = ("dead_lanes_counted", "last_slot_gradient_dropped", "t0_ignored", "lead_time_of_scenario_0", "lost_clamp_missing_in_backward",
           "detach_input_ignored", "holding_cost_on_backlog", "top_link_uses_on_hand")


def emulate(c, defect=None, width=32, dtype=torch.float32):
    """The same rollout written the kernels' way - one (B, F) state block, pipelines shifted in place, orders placed through a
    one-hot of the lead time - in float32, with its own env step (not the oracle's).  `defect`: one of DEFECTS, planted.  `width`
    only matters to "dead_lanes_counted": the lanes past B of the last wavefront replay scenario 0 and are summed into the
    parameter gradients."""
    assert defect is None or defect in DEFECTS
    k = make_inputs(c)
    B, T = c.B, c.T
    Fd, n_out, _ = dims_of(c)
    idx = torch.arange(B)
    if defect == "dead_lanes_counted":
        idx = torch.cat([idx, torch.zeros(-(-B // width) * width - B, dtype=torch.long)])
    n = idx.numel()
    f = lambda x: x.to(dtype)[idx]   # noqa: E731
    data = {name: f(v) for name, v in k["data"].items()}
    g_reward = f(effective_g_reward(c))
    lead_of = lambda t: (t[:1].expand_as(t) if defect == "lead_time_of_scenario_0" else t).long()   # noqa: E731
    params = [(W.to(dtype).clone().requires_grad_(True), b.to(dtype).clone().requires_grad_(True)) for W, b in k["layers"]]
    probes = [torch.zeros(W.shape[0], T, n, dtype=dtype, requires_grad=True) for W, _ in params]
    init = [data["initial_inventories"].flatten(1)]
    if c.head == 1:
        init.append(data["initial_warehouse_inventories"].flatten(1))
    if c.E:
        init.append(data["initial_echelon_inventories"].flatten(1))
    st = torch.cat(init, dim=1)
    seg = segments(c)
    p, hc = data["underage_costs"][:, 0], data["holding_costs"][:, 0]
    leads = [lead_of(data["lead_times"][:, 0, 0])]
    if c.head == 1:
        leads.append(lead_of(data["warehouse_lead_times"][:, 0]))
        leads += [lead_of(data["echelon_lead_times"][:, e]) for e in range(c.E)]

    def shift(st, o, W, after, a, lead):
        cols = []
        for s in range(W - 1):
            nxt = st[:, o + s + 1]
            if defect == "last_slot_gradient_dropped" and s + 1 == W - 1:
                nxt = nxt.detach()
            cols.append(after + nxt if s == 0 else nxt)
        cols.append(torch.zeros_like(after))
        placed = (torch.arange(W)[None] == (lead - 1)[:, None]).to(dtype) * (a * (a != 0))[:, None]   # a zero order is not placed
        return torch.stack(cols, dim=1) + placed

    hist = {name: [] for name in ("states_hist", "hidden_hist", "logits_hist", "rewards")}
    loss = 0
    for t in range(T):
        hist["states_hist"].append(_rows(st))
        detach = c.detach and defect != "detach_input_ignored"
        h, hid = (st.detach() if detach else st), []
        for i, (W, b) in enumerate(params[:-1]):
            h = F.elu(h @ W.t() + b + probes[i][:, t].t())
            hid.append(_rows(h))
        z = h @ params[-1][0].t() + params[-1][1] + probes[-1][:, t].t()
        hist["hidden_hist"].append(torch.cat(hid, dim=0))
        hist["logits_hist"].append(_rows(z))
        d = data["demands"][:, 0, t if defect == "t0_ignored" else c.t0 + t]
        on_hand = st[:, 0]
        after = on_hand - d
        holding = hc * (after if defect == "holding_cost_on_backlog" else torch.relu(after))
        cost = -p * torch.minimum(on_hand, d) + holding if c.profit else p * torch.relu(-after) + holding
        if c.lost:
            clamped = torch.relu(after)
            after = after + (clamped - after).detach() if defect == "lost_clamp_missing_in_backward" else clamped
        if c.head == 0:
            order = F.softplus(z[:, 0] + 1)
            order = torch.round(order) if c.round_orders else order
            nxt = [shift(st, 0, c.Ws, after, order, leads[0])]
        else:
            top = seg[2][0] if c.E else seg[1][0]
            ups = [st[:, top] if defect == "top_link_uses_on_hand" else torch.full((n,), UPPER_BOUND, dtype=dtype)]
            ups += [st[:, o] for o, _ in seg[2:]] + [st[:, seg[1][0]]]
            a = [torch.sigmoid(z[:, j]) * ups[j] for j in range(c.E + 2)]   # [echelons..., warehouse, store]
            a = [torch.round(v) for v in a] if c.round_orders else a
            nxt = [shift(st, 0, c.Ws, after, a[-1], leads[0])]
            w_after = st[:, c.Ws] - a[-1]
            cost = cost + data["warehouse_holding_costs"][:, 0] * torch.relu(w_after)
            if c.edge:
                cost = cost + data["warehouse_edge_costs"][:, 0] * a[c.E]
            nxt.append(shift(st, c.Ws, c.Ww, w_after, a[c.E], leads[1]))
            for e in range(c.E):
                o = seg[2 + e][0]
                e_after = st[:, o] - a[e + 1]   # echelon e ships what echelon e + 1 (the last: the warehouse) ordered
                cost = cost + data["echelon_holding_costs"][:, e] * torch.relu(e_after)
                nxt.append(shift(st, o, c.We, e_after, a[e], leads[2 + e]))
        hist["rewards"].append(cost.detach())
        loss = loss + (g_reward * cost).sum()
        st = torch.cat(nxt, dim=1)
    res = _finish(c, hist, st, loss, params, probes, None, None, None)
    return {name: (v[..., :B] if name in FORWARD_QUANTITIES + DZ_QUANTITIES else v) for name, v in res.items()}


# ---- the checker -------------------------------------------------------------------------------------------------------------------
def as_rows(name, x):
    """a quantity as (rows, elements of the row, B): rewards are one row, the final state one row per state row, a parameter
    gradient tensor one row"""
    if name == "rewards":
        return x.reshape((1,) + tuple(x.shape))
    if name == "state_final":
        return x.unsqueeze(1)
    if name.startswith("g_"):
        return x.reshape(1, -1, 1)
    return x


def row_errors(name, got, want, cols=None):
    """e(row) = max|got - want| / max|want row| over the scenarios `cols` (a bool mask; all when None).  Rows that are identically
    zero in `want` are left out (`zero_rows`: the kernel has to give exact zeros there).  Returns (worst e, its row)."""
    g, w = as_rows(name, got), as_rows(name, want)
    assert g.shape == w.shape, (name, g.shape, w.shape)
    if cols is not None:
        g, w = g[..., cols], w[..., cols]
    if w.numel() == 0:
        return 0.0, -1
    scale = w.abs().flatten(1).max(dim=1).values
    err = (g - w).abs().flatten(1).max(dim=1).values
    nz = scale > 0
    if not nz.any():
        return 0.0, -1
    e = torch.where(nz, err / torch.where(nz, scale, torch.ones_like(scale)), torch.zeros_like(err))
    e = torch.nan_to_num(e, nan=float("inf"))
    i = int(e.argmax())
    return float(e[i]), i


def zero_rows(name, want, cols=None):
    w = as_rows(name, want)
    if cols is not None:
        w = w[..., cols]
    return w.abs().flatten(1).max(dim=1).values == 0 if w.numel() else torch.zeros(w.shape[0], dtype=torch.bool)


def cols_of(c, name):
    """the scenarios quantity `name` is compared on (None: all)"""
    if name in DZ_QUANTITIES:
        return kept(c)
    if name.startswith("g_"):
        return None   # (summed over the scenarios: the knife edges carry a zero g_reward instead)
    return forward_cols(c)


@functools.lru_cache(maxsize=None)
def yardstick(c):
    """{quantity: worst-row e32}: the float32 run of the reference against the float64 run, on the columns each is compared on"""
    r64, r32 = reference(c, torch.float64), reference(c, torch.float32)
    names = FORWARD_QUANTITIES + (() if c.round_orders else DZ_QUANTITIES + param_quantities(c))
    return {n: row_errors(n, r32[n], r64[n], cols_of(c, n))[0] for n in names}


def bar(e32):
    return max(BAR_FACTOR * e32, BAR_FLOOR)


def check(c, got, tag="", out=print):
    """Every quantity in `got` (float64, the reference's layouts) against the float64 reference and the bar.  Returns
    (failures, {quantity: e / e32}); every figure goes through `out` before anything is judged."""
    r64, e32 = reference(c, torch.float64), yardstick(c)
    failures, ratios = [], {}
    for n, x in got.items():
        cols = cols_of(c, n)
        e, row = row_errors(n, x, r64[n], cols)
        zero = zero_rows(n, r64[n], cols)
        g = as_rows(n, x)
        g = g if cols is None else g[..., cols]
        ratios[n] = e / e32[n] if e32[n] > 0 else (0.0 if e == 0 else float("inf"))
        out(f"{c.id:16s} {tag:8s} {n:12s} e {e:.2e} (row {row})  e32 {e32[n]:.2e}  ratio {ratios[n]:.2f}  bar {bar(e32[n]):.2e}  "
            f"zero rows {int(zero.sum())}")
        if not bool((g[zero] == 0).all()):
            failures.append((n, "a row that is identically zero in the reference is not exactly zero"))
        if not e <= bar(e32[n]):
            failures.append((n, f"e {e:.3e} at row {row} above the bar {bar(e32[n]):.3e} (e32 {e32[n]:.3e})"))
    return failures, ratios


# ---- descriptor and buffers of one launch (device-agnostic: the host build of the bodies takes the same) ----------------------------
class Buf:
    """`rows` rows of [T][ldb] floats (the kernels' history layout) in a buffer that is NaN everywhere, with a NaN tail"""
    TAIL = 64

    def __init__(self, rows, T, ldb, B, dev, pad=None):
        self.rows, self.T, self.ldb, self.B = rows, T, ldb, B
        self.buf = torch.full((rows * T * ldb + self.TAIL,), NAN, device=dev)
        if pad is not None:   # (rewards: the padding columns are the caller's zeros, which nic_small_rollout_reduce sums)
            self.view()[:, :, B:] = pad
        self.pad = pad

    def view(self):
        return self.buf[:self.rows * self.T * self.ldb].view(self.rows, self.T, self.ldb)

    def get(self):
        return self.view()[:, :, :self.B].cpu().double()

    def outside_untouched(self):
        """bit for bit what it was outside (row < rows, t < T, b < B)"""
        rest = self.buf.clone()
        rest[:self.rows * self.T * self.ldb].view(self.rows, self.T, self.ldb)[:, :, :self.B] = NAN
        want = Buf(self.rows, self.T, self.ldb, self.B, self.buf.device, self.pad).buf
        return torch.equal(rest.view(torch.int32), want.view(torch.int32))

    def untouched(self):
        return bool(torch.isnan(self.buf).all())


def prepare(c, width, dev):
    """descriptor + every buffer of one case at `width` scenarios per wavefront (0: the default, 32); inputs carry NaN wherever the
    kernels must not look"""
    k = make_inputs(c)
    Fd, n_out, P = dims_of(c)
    B, T, ld = c.B, c.T, c.ldb
    L = types.SimpleNamespace(case=c, width=width, P=P)
    prob = EnvProblem(k["problem"], {n: v.to(dev) for n, v in k["data"].items()}, dev)
    for name in ("underage", "holding", "lead", "wh_holding", "wh_lead", "wh_edge", "ech_holding", "ech_lead"):
        tab = getattr(prob, name)   # the case's choice of table layout took
        if tab.tensor is not None and B > 1:
            assert (tab.scn_stride == 1) == c.per_scenario, (c.id, name)
    head = "serial" if c.head else "softplus"
    dims = [Fd] + [H] * c.n_hidden + [n_out]
    assert sr.SmallRolloutPlan.supports(prob, head, dims), c.id
    plan = sr.SmallRolloutPlan(prob, head, dims)
    L.weights = torch.full((P + 5,), NAN, device=dev)
    L.weights[:P] = torch.cat([t.reshape(-1) for wb in k["layers"] for t in wb]).to(dev)
    n_dem = k["data"]["demands"].shape[2]
    assert n_dem > c.t0 + T
    L.demand = torch.full((n_dem, 1, ld), NAN, device=dev)
    L.demand[:, :, :B] = k["data"]["demands"].permute(2, 1, 0).to(dev)
    init = [k["data"]["initial_inventories"].flatten(1)]
    if c.head == 1:
        init.append(k["data"]["initial_warehouse_inventories"].flatten(1))
    if c.E:
        init.append(k["data"]["initial_echelon_inventories"].flatten(1))
    L.state0 = torch.full((Fd, ld), NAN, device=dev)
    L.state0[:, :B] = torch.cat(init, dim=1).t().to(dev)
    d = plan.desc(T, c.t0, L.weights, L.demand, L.state0, UPPER_BOUND, round_orders=bool(c.round_orders), prob=prob, lane_scenarios=width)
    d.ldb, d.detach_input = ld, c.detach   # (EnvProblem pads to 64 columns; its tables keep their own strides)
    assert (d.Ws, d.Wn, d.Ww, d.E, d.We, d.F, d.n_out) == (c.Ws, int(c.head == 1), c.Ww, c.E, c.We, Fd, n_out)
    L.desc, L.keep = d, (prob, plan)
    L.rewards = Buf(1, T, ld, B, dev, pad=0.0)
    L.state_final = Buf(Fd, 1, ld, B, dev)
    w16 = width == 16
    # (NIC_SR16_STATE_ROWS / NIC_SR16_LOGIT_ROWS of include/nic_rollout.h)
    rows = ((Fd + 3) // 4 * 4 if w16 else Fd, H * c.n_hidden, (1 if n_out == 1 else (n_out + 3) // 4 * 4) if w16 else n_out)
    L.hist = [Buf(r, T, ld, B, dev) for r in rows]
    L.dz_hidden, L.dz_out = Buf(H * c.n_hidden, T, ld, B, dev), Buf(n_out, T, ld, B, dev)
    g = effective_g_reward(c)
    if c.g_uniform:
        assert bool(kept(c).all()), (c.id, "a uniform g_reward cannot leave a scenario out")
        L.g_reward = Table(g[:1].contiguous().to(dev), 0, 0)
    else:
        gt = torch.full((ld,), NAN, device=dev)
        gt[:B] = g.to(dev)
        L.g_reward = Table(gt, 0, 1)
    L.slab_rows = -(-B // 16)   # nic_small_rollout_bwd_wgrad_slots
    L.slab = torch.full((L.slab_rows + 1, P + 3), NAN, device=dev)
    return L
