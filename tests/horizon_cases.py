"""The whole-horizon kernels (csrc/horizon_rollout.hip) against a plain torch rollout in float64: case table, inputs, reference.

CPU only (torch + the oracle's env step).  tests/test_horizon_cases_host.py checks the conditions on the inputs from the reference
alone; tests/test_gpu_horizon.py launches `nic_horizon_rollout_fwd / _bwd` through the C ABI on the same table and compares every
output element by element.

The reference rolls T periods of
    z1 = W1[:, :FD] @ state + z1_obs[:, t];  h1 = ELU(z1);  z2 = W2 h1 + b2;  h2 = ELU(z2);  z3 = W3 h2 + b3
    orders = data_driven head(z3): ReLU, adjacency mask, proportional allocation against each warehouse's whole pipeline
    oracle.env_step (drop mode: an order on a pair without a lead time arrives nowhere)
with state rows [store pipelines | warehouse pipelines] and loss = sum_t sum_b g_reward[b] * reward[t, b].  The pre-activation
gradients are autograd's: d loss / d z1_obs, and the gradients of zero-valued probes added to z2 and z3 (mode 2: of the level tape).

Bar (tests/test_gpu_horizon.py): per quantity, row by row, e(row) = max|x - ref64| / max|ref64 row|; a quantity passes when its
worst row has e_kernel <= max(10 * worst-row e32, 2e-6), e32 being the float32 run of this very reference.  Gradients are compared
on the scenarios whose smallest decision margin exceeds 1e-4 (`KNIFE_EDGE`), forward quantities on all scenarios.
"""
import functools
from collections import namedtuple

import torch
import torch.nn.functional as F

from oracle import inventory_oracle as orc

KNIFE_EDGE = 1e-4        # (the threshold _order_up_to_knife_edges uses)
MAX_EXCLUDED = 0.25      # at most a quarter of a case's scenarios may be knife edges
BAR_FACTOR, BAR_FLOOR = 10.0, 2e-6

HCase = namedtuple("HCase", "id seed S Wn Ws Ww B T t0 H1 H2 profit lost edge per_scenario g_uniform ldb hist_gap w_gap kind0 "
                            "mode allow_negative")


def C(id, seed, S, Wn, Ws, Ww, B, T, t0=0, H1=32, H2=32, profit=False, lost=True, edge=True, per_scenario=False, g_uniform=False,
      ldb=64, hist_gap=0, w_gap=0, kind0=0, mode=0, allow_negative=0):
    assert ldb % 16 == 0 and ldb >= B
    return HCase(id, seed, S, Wn, Ws, Ww if Wn else 0, B, T, t0, H1, H2, profit, lost, edge and Wn > 0, per_scenario, g_uniform, ldb,
                 hist_gap, w_gap, kind0, mode, allow_negative)


# Shapes: every instantiation, every threshold of fwd_steps / bwd_variant from both sides, the limits nic_horizon_rollout_ok admits.
# Measured on one MI355X, worst e_kernel / e32 over the cases and quantities, per instantiation (bar: 10):
#   horizon_fwd_kernel<8,16> 2.21 (orders-S7, rewards)   <8,40> 3.76 (FD65)   <8,64> 7.76 (max, one final-state row of small maximum)
#   horizon_bwd_kernel<8,0>  1.31 (nout16)               <8,1>  1.48 (FD65)   <8,2>  2.24 (S64-Wn0)
# Planted arithmetic faults and the cases they turn red: DESIGN.md, "Whole-horizon kernels against a float64 rollout".
HORIZON_CASES = [
    C("min", 21, 1, 0, 2, 0, B=1, T=3, H1=1, H2=1, ldb=16, hist_gap=8),
    C("stores-only", 12, 5, 0, 8, 0, B=17, T=4, t0=2, H1=24, H2=8, ldb=48, w_gap=3, per_scenario=True, lost=False),
    C("nout16", 13, 7, 2, 8, 2, B=16, T=4, ldb=16, hist_gap=48, g_uniform=True),
    C("FD64", 14, 8, 1, 7, 8, B=33, T=3, t0=2, H1=32, H2=48, kind0=1, per_scenario=True, profit=True),
    C("FD65", 15, 9, 1, 7, 2, B=17, T=5, H1=64, H2=17, kind0=0, ldb=32, w_gap=5, edge=False),
    C("FD160", 16, 26, 2, 6, 2, B=33, T=3, H1=48, H2=40, ldb=48, per_scenario=True),
    C("FD161", 17, 31, 2, 5, 3, B=17, T=4, t0=2, H1=40, H2=64, hist_gap=8, profit=True, g_uniform=True),
    C("nout80", 18, 19, 4, 2, 2, B=33, T=4, H1=64, H2=64, w_gap=1, lost=False),
    C("nout81", 19, 26, 3, 2, 2, B=17, T=3, H1=33, H2=47, ldb=32, per_scenario=True, kind0=1),
    C("max", 20, 31, 4, 8, 2, B=33, T=3, t0=2, H1=64, H2=64, ldb=48, hist_gap=8, w_gap=7, per_scenario=True),
    C("S64-Wn1", 21, 64, 1, 3, 8, B=17, T=4, H1=56, H2=24, kind0=1, profit=True, edge=False),
    C("S64-Wn0", 22, 64, 0, 4, 0, B=40, T=3, H1=64, H2=31, ldb=48, per_scenario=True, g_uniform=True),
    C("Wn32", 23, 3, 32, 2, 7, B=17, T=5, t0=2, H1=48, H2=64, ldb=32, hist_gap=48),
    C("Wn9", 24, 5, 9, 3, 4, B=33, T=4, H1=40, H2=33, w_gap=2, per_scenario=True, lost=False),
    C("ref", 25, 21, 3, 6, 3, B=40, T=5, t0=2, H1=32, H2=32, per_scenario=True),
]
# tape modes: levels (2, with a backward) or orders (1, forward only) drawn per (row, t, b) by the same generator
TAPE_CASES = [
    C("levels-S5", 31, 5, 0, 8, 0, B=17, T=4, t0=2, mode=2, ldb=32, hist_gap=8, per_scenario=True),
    C("levels-S5-neg", 32, 5, 0, 8, 0, B=33, T=3, mode=2, allow_negative=1, lost=False, g_uniform=True),
    C("levels-S64", 33, 64, 0, 4, 0, B=40, T=3, mode=2, ldb=48, profit=True),
    C("levels-S64-neg", 34, 64, 0, 4, 0, B=17, T=4, t0=2, mode=2, allow_negative=1, per_scenario=True),
    # a pipeline shorter than the horizon: an order on the longest lead time still comes on hand, so the level's gradient through
    # the LAST pipeline slot is not zero (with T <= Ws + 1 it is: dropping that term went unnoticed on the four cases above)
    C("levels-Ws2", 37, 6, 0, 2, 0, B=33, T=5, mode=2, ldb=48, hist_gap=8, per_scenario=True),
    C("orders-S7", 35, 7, 2, 8, 2, B=17, T=4, mode=1, ldb=32, per_scenario=True),
    C("orders-S31", 36, 31, 4, 8, 2, B=33, T=3, t0=2, mode=1, hist_gap=8),
]
ALL_CASES = HORIZON_CASES + TAPE_CASES
CASE_IDS = [c.id for c in ALL_CASES]
assert len(set(CASE_IDS)) == len(CASE_IDS)


def dims_of(c):
    """(FD, n_out, n_ord): state rows, logits rows, order rows (the order history carries Wn more: what each warehouse shipped)"""
    nsup = max(c.Wn, 1)
    return c.S * c.Ws + c.Wn * c.Ww, (c.Wn + c.S * c.Wn if c.Wn else c.S), c.S * nsup + c.Wn


def expected_kernels(c):
    """names nic_last_kernel() reports after the forward / the backward launch (horizon_rollout.hip: fwd_steps, bwd_variant)"""
    FD, n_out, _ = dims_of(c)
    steps = 16 if FD <= 64 else (40 if FD <= 160 else 64)
    var = 0 if (FD <= 64 and n_out <= 16) else (1 if (FD <= 192 and n_out <= 80) else 2)
    return f"horizon_fwd_kernel<8,{steps}>", f"horizon_bwd_kernel<8,{var}>"


ALL_KERNELS = {f"horizon_fwd_kernel<8,{s}>" for s in (16, 40, 64)} | {f"horizon_bwd_kernel<8,{v}>" for v in (0, 1, 2)}


def _uniform(gen, shape, lo, hi):
    return lo + (hi - lo) * torch.rand(shape, generator=gen)


def _table(gen, B, shape, lo, hi, per_scenario, integer=False):
    """(B, *shape) static table: per scenario, or one row behind an `expand` view (stride 0) as the reference's"""
    n = B if per_scenario else 1
    t = torch.randint(int(lo), int(hi) + 1, (n,) + shape, generator=gen).float() if integer else _uniform(gen, (n,) + shape, lo, hi)
    return t if per_scenario else t.expand((B,) + shape)


@functools.lru_cache(maxsize=None)
def make_inputs(c):
    """Everything a launch reads, float32 on the CPU, in the reference's logical shapes ((B, ...) data, (rows, T, B) tapes).

    Continuous draws (no planted ties: the knife edges are measured and excluded, not constructed).  Warehouses alternate between
    two kinds: RICH ones hold about 40 S T / Ww per slot and never bind; TIGHT ones hold 0.1 S in all (their stores ask for about 0.3 S a period) and bind from
    the first period in two scenarios of three (in the third they hold 3 S per slot, enough for the horizon, so that no state row
    is rounding noise in every scenario), have lead times >= 2 and a bias of +0.08 S with small weights on their own-order logit - a warehouse whose allocation binds ships its whole
    pipeline total, and with a zero own order or a lead time of 1 its on-hand stock would equal what it ships up to the 1e-10 of
    the allocation's denominator.  First-layer columns are scaled by the inverse of their state row's typical magnitude."""
    gen = torch.Generator().manual_seed(c.seed)
    B, S, Wn, Ws, Ww, T = c.B, c.S, c.Wn, c.Ws, c.Ww, c.T
    nsup = max(Wn, 1)
    FD, n_out, n_ord = dims_of(c)
    ps = c.per_scenario
    problem = {"n_stores": S, "n_warehouses": Wn, "n_extra_echelons": 0, "lost_demand": c.lost, "maximize_profit": c.profit}
    data = {"demands": _uniform(gen, (B, S, c.t0 + T + 1), 0.5, 6.0), "underage_costs": _table(gen, B, (S,), 2.0, 9.0, ps),
            "holding_costs": _table(gen, B, (S,), 0.2, 2.0, ps), "initial_inventories": _uniform(gen, (B, S, Ws), 0.0, 4.0)}
    mask = None
    lead = _table(gen, B, (S, nsup), 1, Ws, ps, integer=True)
    if Wn:
        mask = (torch.rand(S, Wn, generator=gen) < 0.75).float()
        for w in range(Wn):   # every warehouse serves somebody
            if mask[:, w].sum() == 0:
                mask[w % S, w] = 1.0
        lead = (lead.clone() if ps else lead[:1].clone()) * mask[None]   # pairs without an edge: lead time 0
        lead = lead if ps else lead.expand(B, S, nsup)
    data["lead_times"] = lead
    typ = torch.full((FD,), 2.0)
    tight = torch.zeros(max(Wn, 1), dtype=torch.bool)
    if Wn:
        tight = torch.tensor([(w + c.kind0) % 2 == 1 for w in range(Wn)]) & (c.mode == 0)
        rich_slot = 40.0 * S * T / Ww
        scale = torch.full((B, Wn), rich_slot)
        if c.mode == 0:
            scale[:, tight] = 0.1 * S / Ww
            scale[2::3, tight] = 3.0 * S   # (every third scenario: enough for the horizon)
        else:                            # an order tape does not look at the pipeline: on-hand stock on both sides of what is shipped
            scale[:] = 0.6 * S
        data["initial_warehouse_inventories"] = _uniform(gen, (B, Wn, Ww), 0.5, 1.5) * scale[:, :, None]
        data["warehouse_holding_costs"] = _table(gen, B, (Wn,), 0.1, 1.0, ps)
        wl = _table(gen, B, (Wn,), 1, Ww, ps, integer=True)
        wl = wl.clone() if ps else wl[:1].clone()
        wl[:, tight] = torch.clamp(wl[:, tight], min=2.0)
        data["warehouse_lead_times"] = wl if ps else wl.expand(B, Wn)
        if c.edge:
            data["warehouse_edge_costs"] = _table(gen, B, (Wn,), 0.1, 1.0, ps)
        for w in range(Wn):
            typ[S * Ws + w * Ww:S * Ws + (w + 1) * Ww] = max(2.0, 1.5 * S) if tight[w] else rich_slot
    g_reward = _uniform(gen, (1,) if c.g_uniform else (B,), 0.2, 1.2) * (1 - 2 * (torch.rand(1 if c.g_uniform else B, generator=gen) < 0.3).float())
    k = dict(case=c, problem=problem, data=data, mask=mask, g_reward=g_reward.expand(B) if c.g_uniform else g_reward, tight=tight)
    if c.mode == 0:
        H1, H2 = c.H1, c.H2
        W1 = torch.zeros(H1, FD + c.w_gap)   # (the columns beyond FD stand for the observation rows: contracted outside, never read)
        W1[:, :FD] = torch.randn(H1, FD, generator=gen) / (FD ** 0.5) / typ[None]
        W1[:, FD:] = float("nan")
        W2 = torch.full((H2, H1 + c.w_gap), float("nan"))
        W2[:, :H1] = torch.randn(H2, H1, generator=gen) * (1.0 / H1 ** 0.5)
        W3 = torch.full((n_out, H2 + c.w_gap), float("nan"))
        W3[:, :H2] = torch.randn(n_out, H2, generator=gen) * (1.5 / H2 ** 0.5)
        b2, b3 = torch.randn(H2, generator=gen) * 0.3, torch.randn(n_out, generator=gen) * 0.5
        for w in range(Wn):
            if tight[w]:   # its own order is always positive, and about a quarter of what its stores ask for
                b3[w] = 0.08 * S
                W3[w, :H2] *= 0.1 * b3[w]
        k.update(W1=W1, W2=W2, W3=W3, b2=b2, b3=b3, z1_obs=torch.randn(H1, T, B, generator=gen) * 0.5)
    elif c.mode == 2:   # order-up-to levels around the pipeline total (both sides of the clip)
        k["tape"] = _uniform(gen, (S, T, B), 0.6, 1.6) * (2.0 * Ws)
    else:
        tape = _uniform(gen, (n_ord, T, B), 0.0, 3.0)
        tape[torch.rand(n_ord, T, B, generator=gen) < 0.25] = 0.0
        k["tape"] = tape
    return k


_OBS = {"include_static_features": {"holding_costs": True, "underage_costs": True, "lead_times": True},
        "include_days_to_christmas": False, "time_features": None, "sample_features": None}


def _rows(x):
    """(B, rows) of one period -> (rows, B)"""
    return x.detach().t()


@functools.lru_cache(maxsize=None)
def reference(c, dtype):
    """The rollout of case `c` in `dtype` (torch.float64: the referee; torch.float32: the yardstick of the bar).  Returns float64
    tensors in the kernels' layouts - histories (rows, T, B), rewards (T, B), state_final (FD, B) - plus, per scenario, the
    smallest decision margin over all periods and the counts the host test asserts.  Computed once per session, never modified."""
    k = make_inputs(c)
    B, S, Wn, Ws, Ww, T = c.B, c.S, c.Wn, c.Ws, c.Ww, c.T
    nsup = max(Wn, 1)
    FD, n_out, n_ord = dims_of(c)
    f = lambda x: x.to(dtype)   # noqa: E731
    data = {n: f(v) for n, v in k["data"].items()}
    env = orc.env_reset(T, k["problem"], data, dict(_OBS, demand={"past_periods": 0, "period_shift": c.t0},
                                                     include_warehouse_inventory=Wn > 0))
    env.zero_lead_orders = "drop"
    mask = f(k["mask"]) if Wn else None
    g_reward = f(k["g_reward"])
    if c.mode == 0:
        W1, W2, W3 = f(k["W1"][:, :FD]), f(k["W2"][:, :c.H1]), f(k["W3"][:, :c.H2])
        b2, b3 = f(k["b2"]), f(k["b3"])
        z1_obs = f(k["z1_obs"]).requires_grad_(True)
        p2 = torch.zeros(c.H2, T, B, dtype=dtype, requires_grad=True)
        p3 = torch.zeros(n_out, T, B, dtype=dtype, requires_grad=True)
    else:
        tape = f(k["tape"]).requires_grad_(c.mode == 2)
    hist = {n: [] for n in ("state_hist", "h1_hist", "h2_hist", "logits_hist", "orders_hist", "rewards")}
    margins = {}   # kind of decision -> (B,) smallest margin over the periods
    stats = dict(bind=0, free=0, logit_pos=0, logit_neg=0, clip_on=0, clip_off=0)

    def note(kind, m):   # m: (B, ...) margins of one decision
        if m.numel():
            m = m.detach().double().reshape(B, -1).min(dim=1).values
            margins[kind] = torch.minimum(margins[kind], m) if kind in margins else m

    loss = 0
    for t in range(T):
        st = env.obs["store_inventories"]
        wh = env.obs["warehouse_inventories"] if Wn else None
        x = torch.cat([st.flatten(1)] + ([wh.flatten(1)] if Wn else []), dim=1)   # (B, FD)
        hist["state_hist"].append(_rows(x))
        wo = None
        if c.mode == 0:
            h1 = F.elu(x @ W1.t() + z1_obs[:, t].t())
            h2 = F.elu(h1 @ W2.t() + b2 + p2[:, t].t())
            z3 = h2 @ W3.t() + b3 + p3[:, t].t()
            for n, v in (("h1_hist", h1), ("h2_hist", h2), ("logits_hist", z3)):
                hist[n].append(_rows(v))
            out = torch.relu(z3)
            if Wn:
                live = torch.cat([torch.ones(Wn, dtype=torch.bool), mask.flatten() > 0])
                wo = out[:, :Wn]
                alloc = out[:, Wn:].reshape(B, S, Wn) * mask[None]
                ratio = wh.sum(dim=2) / (alloc.sum(dim=1) + 1e-10)
                stores = alloc * torch.clip(ratio, max=1.0)[:, None, :]
                note("allocation", (ratio - 1).abs())
                stats["bind"] += int((ratio < 1).sum())
                stats["free"] += int((ratio >= 1).sum())
            else:
                live = torch.ones(n_out, dtype=torch.bool)
                stores = out.unsqueeze(2)
            zl = z3.detach()[:, live]
            note("logit", zl.abs())
            stats["logit_pos"] += int((zl > 0).sum())
            stats["logit_neg"] += int((zl < 0).sum())
        elif c.mode == 2:
            level = tape[:, t].t()
            a = level - st.sum(dim=2)
            if not c.allow_negative:
                note("level", (a / (1 + level.abs())).abs())
                stats["clip_on"] += int((a < 0).sum())
                stats["clip_off"] += int((a >= 0).sum())
                a = torch.clip(a, min=0)
            stores = a.unsqueeze(2)
        else:
            rows = tape[:, t].t()
            stores, wo = rows[:, :S * nsup].reshape(B, S, nsup), (rows[:, S * nsup:] if Wn else None)
        action = {"stores": stores}
        d = data["demands"][:, :, c.t0 + t]
        note("store", (st[:, :, 0] - d).abs() / (1 + d))
        orders = [_rows(stores.flatten(1))]
        if Wn:
            action["warehouses"] = wo.unsqueeze(2)
            shipped = stores.sum(dim=1)
            note("warehouse", (wh[:, :, 0] - shipped).abs() / (1 + wh[:, :, 0].abs()))
            orders += [_rows(wo), _rows(shipped)]
        hist["orders_hist"].append(torch.cat(orders, dim=0))
        reward = orc.env_step(env, action)
        hist["rewards"].append(reward.detach())
        loss = loss + (g_reward * reward).sum()
    res = {n: torch.stack(v, dim=1).double() for n, v in hist.items() if v and n != "rewards"}
    res["rewards"] = torch.stack(hist["rewards"], dim=0).double()
    fin = [env.obs["store_inventories"].flatten(1)] + ([env.obs["warehouse_inventories"].flatten(1)] if Wn else [])
    res["state_final"] = _rows(torch.cat(fin, dim=1)).double()
    if c.mode != 1:
        if loss.requires_grad:   # (not when every order of the horizon is zero: the zero filter cuts the graph)
            loss.backward()
        grad = lambda x: (x.grad if x.grad is not None else torch.zeros_like(x)).double()   # noqa: E731
        if c.mode == 0:
            res.update(dz1_hist=grad(z1_obs), dz2_hist=grad(p2), dz3_hist=grad(p3))
        else:
            res["dz3_hist"] = grad(tape)
    for n, v in res.items():
        assert v.dtype == torch.float64
    res["margin"] = torch.stack(list(margins.values())).min(dim=0).values
    res["margins"], res["stats"] = margins, stats
    return res


FORWARD_QUANTITIES = ("rewards", "state_final", "state_hist", "h1_hist", "h2_hist", "logits_hist", "orders_hist")
GRAD_QUANTITIES = ("dz1_hist", "dz2_hist", "dz3_hist")


def kept(c):
    """scenarios whose gradients are compared: every decision of the float64 run clears the knife-edge threshold"""
    return reference(c, torch.float64)["margin"] > KNIFE_EDGE


def as_rows(name, x):
    """a quantity as (rows, elements of the row, B): rewards are one row, the final state one row per state row"""
    if name == "rewards":
        return x.reshape((1,) + tuple(x.shape))
    if name == "state_final":
        return x.unsqueeze(1)
    return x


def row_errors(name, got, want, cols=None):
    """e(row) = max|got - want| / max|want row| over the scenarios `cols` (a bool mask; all of them when None).  Rows that are
    identically zero in `want` are left out here (`zero_rows`: the kernel has to give exact zeros there).  Returns (worst e, its row)."""
    g, w = as_rows(name, got), as_rows(name, want)
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


def yardstick(c):
    """{quantity: worst-row e32}: the float32 run of the reference against the float64 run, on the columns each is compared on"""
    r64, r32 = reference(c, torch.float64), reference(c, torch.float32)
    keep = kept(c)
    return {n: row_errors(n, r32[n], r64[n], keep if n in GRAD_QUANTITIES else None)[0]
            for n in FORWARD_QUANTITIES + GRAD_QUANTITIES if n in r64}


def bar(e32):
    return max(BAR_FACTOR * e32, BAR_FLOOR)
