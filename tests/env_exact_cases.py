"""One period of inventory dynamics on EXACT inputs: the env-step kernels against the oracle bit for bit.

One period is adds, subtracts, compares and products of pairs.  With every input on a coarse dyadic grid (multiples of 1/8, incoming
gradients multiples of 1/4, magnitudes of a few units) every intermediate is a multiple of 1/64 below 2^18 and therefore exactly
representable in float32: no summation order can change a bit, ties are real ties, and the kernel has to EQUAL the oracle - next
state, reward, state gradients, order gradients, tie rules included - with no tolerance and no knife-edge exclusion.  The condition
on the inputs is checked on the reference alone: the oracle in float32 must equal the oracle in float64 bit for bit.

Backend-agnostic like kernel_checks.py: the host build of the NIC_HD bodies (tests/test_env_exact_host.py, CPU) and the product
library through the C ABI (tests/test_gpu_kernels.py, GPU) run the same table.  What the host tier cannot see is the device
wrappers: the LDS exchange, the chunk rounds of kChunk = 8 warehouses, multi-workgroup indexing, the <4|8|16>-slot instantiations.
"""
import functools
from collections import namedtuple

import torch

from kernel_checks import HipBackend, P, _demand_table
from neural_inventory_control_amd import _lib, layout
from neural_inventory_control_amd.layout import EnvProblem, Table, ref_view, to_soa
from oracle import inventory_oracle as orc

EnvCase = namedtuple("EnvCase", "id seed B S Wn E Ws Ww We lost profit edge per_scenario in_place null_grads")


def C(id, seed, B, S, Wn, E, Ws, Ww, We, lost=True, profit=False, edge=True, per_scenario=False, in_place=False, null_grads=()):
    return EnvCase(id, seed, B, S, Wn, E, Ws, Ww if Wn else 0, We if E else 0, lost, profit, edge and Wn > 0, per_scenario, in_place,
                   tuple(null_grads))


# The shapes are the smallest at which each path of env_step.hip / env_step_body.h starts (kQuad = 4 lanes per scenario,
# kStoreBatch = 4 stores per lane and batch, kShipBatch = 8, kSupBatch = 3 suppliers, kChunk = 8 warehouses per barrier round,
# 64 scenarios per workgroup, instantiations for <= 4 / <= 8 / <= 16 slots).  Fixed and listed: nothing is drawn at run time.
ENV_EXACT_CASES = (
    # batch edges (one lane, a ragged / full / just-started second workgroup, a ragged third) on S = 5, Wn = 4
    [C(f"B{B}", 100 + B, B, 5, 4, 0, 3, 4, 0, per_scenario=B % 2 == 1) for B in (1, 63, 64, 65, 130)]
    # suppliers below / at / beyond kSupBatch; chunk rounds wc = 0, 8, 16, 24 and the `i = q; i += kQuad` walk inside a later round
    + [C(f"Wn{Wn}", 200 + Wn, 70, 9, Wn, 0, 4, 3, 0, edge=Wn != 12, per_scenario=Wn in (3, 9, 32)) for Wn in (0, 1, 3, 4, 8, 9, 12, 17, 32)]
    # lanes of a quad without a store, the second store batch of a lane at 17, its second ship batch at 33, past 64
    + [C(f"S{S}", 300 + S, 65, S, 2, 0, 3, 3, 0, per_scenario=S in (4, 17, 70)) for S in (1, 3, 4, 5, 16, 17, 33, 64, 70)]
    # the instantiation is decided by each pipeline type in turn (store, warehouse, echelon)
    + [C(f"slots{a}-{b}-{c}", 400 + 31 * a + 7 * b + c, 66, 6, 5, 2, a, b, c, per_scenario=(a + b + c) % 2 == 1)
       for a, b, c in ((2, 2, 2), (4, 4, 4), (5, 3, 3), (3, 8, 2), (3, 3, 9), (16, 2, 2), (2, 16, 2), (2, 2, 16), (16, 16, 16))]
    # env_wh_orders_sum beyond its first batch of 8, the echelon gradient into more than 8 warehouses
    + [C(f"E{E}-Wn{Wn}", 500 + 40 * E + Wn, 70, 7, Wn, E, 3, 4, 5, per_scenario=Wn == 9) for E in (1, 3) for Wn in (1, 9, 17)]
    # the four (lost demand, profit) combinations, uniform and per-scenario tables, on one mid-size case
    + [C(f"lost{int(lo)}-profit{int(pr)}-{'scn' if ps else 'uni'}", 600, 100, 13, 6, 1, 5, 4, 3, lost=lo, profit=pr, per_scenario=ps)
       for lo in (False, True) for pr in (False, True) for ps in (False, True)]
    + [C("in-place", 700, 130, 21, 9, 2, 6, 5, 4, in_place=True, per_scenario=True),
       C("null-grads", 701, 70, 10, 9, 2, 4, 9, 3, null_grads=("wh", "ech")),
       C("null-grads-store", 702, 65, 6, 2, 0, 3, 3, 0, null_grads=("store", "wh")),
       # no echelons, so that the one-store bodies can be composed on it too: their profit branch and its 0.5 / 0.5 tie rule
       C("profit-Wn5", 703, 66, 7, 5, 0, 3, 3, 0, lost=False, profit=True)]
    # the shapes of the CPU probe that motivated this table
    + [C("probe0", 800, 70, 9, 11, 2, 12, 9, 5), C("probe1", 801, 130, 37, 32, 0, 16, 16, 0, per_scenario=True),
       C("probe2", 802, 65, 5, 4, 3, 3, 5, 16, profit=True), C("probe3", 803, 1, 1, 0, 0, 2, 0, 0),
       C("probe4", 804, 200, 64, 9, 1, 7, 2, 2, lost=False, per_scenario=True), C("probe5", 805, 64, 17, 1, 0, 9, 4, 0, edge=False)]
)
ENV_EXACT_IDS = [c.id for c in ENV_EXACT_CASES]
assert len(set(ENV_EXACT_IDS)) == len(ENV_EXACT_IDS)


def expected_variant(c):
    """the <MAXW> instantiation nic_env_step_fwd / _bwd pick for this case (env_step.hip: max_slots)"""
    m = max(c.Ws, c.Ww if c.Wn else 0, c.We if c.E else 0)
    return 4 if m <= 4 else (8 if m <= 8 else _lib.NIC_MAX_SLOTS)


def _grid(gen, shape, lo, hi, step=8):
    """uniform on {lo, lo + 1/step, ..., hi}"""
    return torch.randint(int(lo * step), int(hi * step) + 1, shape, generator=gen).float() / step


def _table(gen, B, shape, lo, hi, per_scenario, integer=False):
    """a (B, *shape) static table: varying per scenario, or one row behind an `expand` view like the reference's (stride 0)"""
    step = 1 if integer else 8
    if per_scenario:
        return _grid(gen, (B,) + shape, lo, hi, step)
    return _grid(gen, (1,) + shape, lo, hi, step).expand((B,) + shape)


def _set(t, idx, value):
    """write into a table that may be an expand view (every scenario shares the row)"""
    base = t if t.stride(0) != 0 else t[:1]
    base[(slice(None),) + idx] = value


def make_case(seed, B, S, Wn, E, Ws, Ww, We, lost, profit, edge, per_scenario_tables):
    """Problem params, data dict, state, actions, g_out and g_reward of one period on the dyadic grid, with planted ties:
    on-hand == demand (every third scenario, even stores), warehouse on-hand == what it ships (every fourth scenario), zero store /
    warehouse / echelon orders, lead times hitting 1 and the last slot, (store, warehouse) pairs with lead time 0 that carry an order
    (dropped).  Lead times never exceed the pipeline length (beyond it the oracle's flat `put` and the kernel differ by design)."""
    gen = torch.Generator().manual_seed(seed)
    nsup = max(Wn, 1)
    ps = per_scenario_tables
    problem = {"n_stores": S, "n_warehouses": Wn, "n_extra_echelons": E, "lost_demand": lost, "maximize_profit": profit}
    data = {"demands": _grid(gen, (B, S, 1), 0, 6), "underage_costs": _table(gen, B, (S,), 1, 9, ps),
            "holding_costs": _table(gen, B, (S,), 0, 2, ps)}
    state = {"store_inventories": _grid(gen, (B, S, Ws), 0, 5)}
    lead = _table(gen, B, (S, nsup), 1, Ws, ps, integer=True)
    if Wn > 0:   # pairs without an edge: lead time 0 (what the many-warehouse settings ship); their orders below are NOT all zero
        no_edge = torch.rand(lead.shape if ps else (1, S, nsup), generator=gen) < 0.15
        (lead if ps else lead[:1])[no_edge] = 0.0
    _set(lead, (0, 0), 1.0)
    _set(lead, (S - 1, nsup - 1), float(Ws))
    if Wn > 0 and (S // 2, Wn // 2) not in ((0, 0), (S - 1, nsup - 1)):
        _set(lead, (S // 2, Wn // 2), 0.0)
    data["lead_times"] = lead
    act = {"stores": _grid(gen, (B, S, nsup), 0, 3)}
    act["stores"][torch.rand(B, S, nsup, generator=gen) < 0.25] = 0.0
    if Wn > 0 and (S // 2, Wn // 2) not in ((0, 0), (S - 1, nsup - 1)):
        act["stores"][:, S // 2, Wn // 2] = torch.clamp(act["stores"][:, S // 2, Wn // 2], min=0.125)   # an order on the zero-lead pair
    state["store_inventories"][0::3, 0::2, 0] = data["demands"][0::3, 0::2, 0]   # on-hand == demand
    if Wn > 0:
        state["warehouse_inventories"] = _grid(gen, (B, Wn, Ww), 0, 5)
        state["warehouse_inventories"][:, :, 0] *= max(1, S // 2)   # (so that warehouses end on both sides of zero at every S)
        state["warehouse_inventories"][1::4, :, 0] = act["stores"][1::4].sum(dim=1)   # post-shipping on-hand exactly 0
        data["warehouse_holding_costs"] = _table(gen, B, (Wn,), 0, 2, ps)
        wl = _table(gen, B, (Wn,), 1, Ww, ps, integer=True)
        _set(wl, (0,), 1.0)
        _set(wl, (Wn - 1,), float(Ww))
        data["warehouse_lead_times"] = wl
        if edge:
            data["warehouse_edge_costs"] = _table(gen, B, (Wn,), 0, 2, ps)
        act["warehouses"] = _grid(gen, (B, Wn, 1), 0, 6)
        act["warehouses"][torch.rand(B, Wn, 1, generator=gen) < 0.2] = 0.0
    if E > 0:
        state["echelon_inventories"] = _grid(gen, (B, E, We), 0, 5)
        state["echelon_inventories"][:, E - 1, 0] *= max(1, Wn // 2)
        data["echelon_holding_costs"] = _table(gen, B, (E,), 0, 2, ps)
        el = _table(gen, B, (E,), 1, We, ps, integer=True)
        _set(el, (0,), 1.0)
        _set(el, (E - 1,), float(We))
        data["echelon_lead_times"] = el
        act["echelons"] = _grid(gen, (B, E, 1), 0, 9)
        act["echelons"][torch.rand(B, E, 1, generator=gen) < 0.2] = 0.0
        state["echelon_inventories"][2::4, E - 1, 0] = act["warehouses"][2::4].sum(dim=(1, 2))   # last echelon ships its stock exactly
    data["initial_inventories"] = state["store_inventories"]
    if Wn > 0:
        data["initial_warehouse_inventories"] = state["warehouse_inventories"]
    if E > 0:
        data["initial_echelon_inventories"] = state["echelon_inventories"]
    g_out = {k: _grid(gen, v.shape, -2, 2, 4) for k, v in state.items()}
    g_reward = _grid(gen, (B,), -2, 2, 4)
    return dict(problem=problem, data=data, state=state, act=act, g_out=g_out, g_reward=g_reward)


def planted(k):
    """which of the planted situations a generated case really contains (the host tier asserts the table covers every one)"""
    c, st, act, d = k["case"], k["state"], k["act"], k["data"]
    lead = d["lead_times"]
    out = {"on_hand_eq_demand": bool((st["store_inventories"][:, :, 0] == d["demands"][:, :, 0]).any()),
           "zero_store_order": bool((act["stores"] == 0).any()), "lead_1": bool((lead == 1).any()),
           "lead_last_slot": bool((lead == c.Ws).any()),
           "zero_lead_with_order": bool(((lead == 0) & (act["stores"] != 0)).any())}
    if c.Wn:
        after = st["warehouse_inventories"][:, :, 0] - act["stores"].sum(dim=1)
        out.update(wh_exactly_empty=bool(((after == 0) & (act["stores"].sum(dim=1) != 0)).any()), wh_short=bool((after < 0).any()),
                   wh_left=bool((after > 0).any()), zero_wh_order=bool((act["warehouses"] == 0).any()))
    if c.E:
        out.update(zero_ech_order=bool((act["echelons"] == 0).any()))
    return out


_OBS = {"include_static_features": {"holding_costs": True, "underage_costs": True, "lead_times": True},
        "demand": {"past_periods": 0, "period_shift": 0}, "include_days_to_christmas": False, "time_features": None,
        "sample_features": None}
_STATE_KEYS = ("store_inventories", "warehouse_inventories", "echelon_inventories")
_ACT_KEYS = ("stores", "warehouses", "echelons")


def oracle_period(k, dtype, null_grads=()):
    """next state, reward, state gradients and order gradients of the oracle's drop mode + autograd in `dtype`"""
    cast = lambda d: {n: v.to(dtype) for n, v in d.items()}   # noqa: E731
    st = {n: v.clone().requires_grad_(True) for n, v in cast(k["state"]).items()}
    act = {n: v.clone().requires_grad_(True) for n, v in cast(k["act"]).items()}
    data = cast(k["data"])
    env = orc.env_reset(1, k["problem"], data, dict(_OBS, include_warehouse_inventory=k["case"].Wn > 0))
    env.obs.update(st)
    env.zero_lead_orders = "drop"
    reward = orc.env_step(env, act)
    g_out = cast(k["g_out"])
    for short, key in zip(("store", "wh", "ech"), _STATE_KEYS):
        if short in null_grads and key in g_out:
            g_out[key] = torch.zeros_like(g_out[key])
    ((reward * k["g_reward"].to(dtype)).sum() + sum((env.obs[n] * g_out[n]).sum() for n in st)).backward()
    grad = lambda x: x.grad if x.grad is not None else torch.zeros_like(x)   # noqa: E731  (all orders 0: the put is skipped)
    res = {"reward": reward.detach()}
    for n in st:
        res["next_" + n] = env.obs[n].detach()
        res["g_" + n] = grad(st[n])
    for n in act:
        res["g_act_" + n] = grad(act[n])
    return res


@functools.lru_cache(maxsize=None)
def reference(c, null_grads=()):
    """The case and its expected values, computed once per session and shared (never modified).  The float32 and the float64 oracle
    must agree bit for bit: that is the condition on the INPUTS, and a case that misses it is a bug of the generator."""
    k = make_case(c.seed, c.B, c.S, c.Wn, c.E, c.Ws, c.Ww, c.We, c.lost, c.profit, c.edge, c.per_scenario)
    k["case"] = c
    r32, r64 = oracle_period(k, torch.float32, null_grads), oracle_period(k, torch.float64, null_grads)
    for n in r32:
        assert r32[n].dtype == torch.float32 and r64[n].dtype == torch.float64
        assert torch.equal(r32[n].double(), r64[n]), (c.id, n, "the oracle is not exact on this input")
    return k, r32


_NAN = float("nan")


def _sentinel(shape, dev):
    return torch.full(shape, _NAN, device=dev)


def _padding_untouched(out, before, B, what):
    """columns [B, ldb) still hold what they held before the launch, compared as bits (both kernels write only under `live`)"""
    assert torch.equal(out[..., B:].contiguous().view(torch.int32), before[..., B:].contiguous().view(torch.int32)), what


def launch_inputs(k, dev, soa_orders):
    """EnvProblem, SoA state, order tables, demand table of a case on `dev`; `keep` holds what the io only has addresses of"""
    c = k["case"]
    prob = EnvProblem(k["problem"], k["data"], dev)
    ld = prob.ldb
    s = to_soa(k["state"]["store_inventories"].to(dev), ld)
    w = to_soa(k["state"]["warehouse_inventories"].to(dev), ld) if c.Wn else None
    e = to_soa(k["state"]["echelon_inventories"].to(dev), ld) if c.E else None
    a = {n: v.to(dev) for n, v in k["act"].items()}
    if soa_orders:   # the engines' dense [S][nsup][ldb] / [Wn][ldb] / [E][ldb] blocks
        so = to_soa(a["stores"], ld)
        ts = Table(so, so.stride(0), 1, so.stride(1))
        tw = Table(to_soa(a["warehouses"][:, :, 0], ld), ld, 1) if c.Wn else None
        te = Table(to_soa(a["echelons"][:, :, 0], ld), ld, 1) if c.E else None
    else:            # scenario-major (B, L, P) tensors as a reference-style policy hands them over
        ts = Table.from_orders(a["stores"])
        tw = Table.from_orders(a["warehouses"][:, :, 0]) if c.Wn else None
        te = Table.from_orders(a["echelons"][:, :, 0]) if c.E else None
    dem = k["data"]["demands"].to(dev)
    return prob, s, w, e, ts, tw, te, _demand_table(dem, 0), (a, dem)


def run_forward(be, k, in_place=False, soa_orders=True):
    c, dev = k["case"], be.device
    prob, s, w, e, ts, tw, te, dem, _keep = launch_inputs(k, dev, soa_orders)
    io = prob.make_io(s, w, e, dem, ts, tw, te)
    if in_place:   # the state buffers are the outputs (env_step_body.h: a batch's rows are read before they are written)
        so, wo, eo = s, w, e
    else:
        so, wo, eo = (_sentinel(x.shape, dev) if x is not None else None for x in (s, w, e))
    r = _sentinel((prob.ldb,), dev)
    before = [x.clone() if x is not None else None for x in (so, wo, eo, r)]
    be.env_fwd(io, so, wo, eo, r)
    be.sync()
    if isinstance(be, HipBackend):
        assert be.l.nic_last_kernel().decode() == f"env_step_fwd_kernel<{expected_variant(c)}>"
    for x, b4, what in zip((so, wo, eo, r), before, ("store", "wh", "ech", "reward")):
        if x is not None:
            _padding_untouched(x, b4, c.B, (c.id, "forward padding", what))
    return so, wo, eo, r


def run_backward(be, k, null_grads=(), soa_orders=True):
    c, dev = k["case"], be.device
    prob, s, w, e, ts, tw, te, dem, _keep = launch_inputs(k, dev, soa_orders)
    io = prob.make_io(s, w, e, dem, ts, tw, te)
    ld = prob.ldb
    g = {n: to_soa(v.to(dev), ld) for n, v in k["g_out"].items()}
    gso = None if "store" in null_grads else g["store_inventories"]
    gwo = None if "wh" in null_grads or not c.Wn else g["warehouse_inventories"]
    geo = None if "ech" in null_grads or not c.E else g["echelon_inventories"]
    grs = torch.zeros(ld, device=dev)
    grs[:c.B] = k["g_reward"].to(dev)
    gsi = _sentinel(s.shape, dev)
    gwi = _sentinel(w.shape, dev) if c.Wn else None
    gei = _sentinel(e.shape, dev) if c.E else None
    gas = _sentinel((c.S, prob.nsup, ld), dev)
    gaw = _sentinel((c.Wn, ld), dev) if c.Wn else None
    gae = _sentinel((c.E, ld), dev) if c.E else None
    outs = (gsi, gwi, gei, gas, gaw, gae)
    before = [x.clone() if x is not None else None for x in outs]
    be.env_bwd(io, gso, gwo, geo, layout.Table(grs, 0, 1).t2(), gsi, gwi, gei, gas, gaw, gae)
    be.sync()
    if isinstance(be, HipBackend):
        assert be.l.nic_last_kernel().decode() == f"env_step_bwd_kernel<{expected_variant(c)}>"
    for x, b4, what in zip(outs, before, ("g_store", "g_wh", "g_ech", "g_store_orders", "g_wh_orders", "g_ech_orders")):
        if x is not None:
            _padding_untouched(x, b4, c.B, (c.id, "backward padding", what))
    return outs


def check_env_exact(be, c, in_place=False, null_grads=()):
    """`torch.equal` between the kernel (host build or HIP) and the oracle for everything one period produces.  in_place: the forward
    launch writes into the state buffers it reads, and must give what the out-of-place launch gives.  null_grads: NULL instead of the
    incoming pipeline gradients named ("store" / "wh" / "ech") - the result of zeros there."""
    null_grads = tuple(null_grads)
    k, want = reference(c, null_grads)
    B = c.B
    got = {}
    so, wo, eo, r = run_forward(be, k, soa_orders=c.seed % 2 == 0)
    got["next_store_inventories"], got["next_warehouse_inventories"], got["next_echelon_inventories"] = so, wo, eo
    assert torch.equal(r[:B].cpu(), want["reward"]), (c.id, "reward")
    gsi, gwi, gei, gas, gaw, gae = run_backward(be, k, null_grads, soa_orders=c.seed % 2 == 0)
    got["g_store_inventories"], got["g_warehouse_inventories"], got["g_echelon_inventories"] = gsi, gwi, gei
    got["g_act_stores"] = gas
    for n in want:
        if n == "reward":
            continue
        have = got.get(n)
        if have is None:   # orders of warehouses / echelons: (B, L, 1) upstream, [L][ldb] here
            have = {"g_act_warehouses": gaw, "g_act_echelons": gae}[n].unsqueeze(1)
        assert torch.equal(ref_view(have, B).cpu(), want[n]), (c.id, n)
    if in_place:
        so2, wo2, eo2, r2 = run_forward(be, k, in_place=True, soa_orders=c.seed % 2 == 0)
        for a, b_, what in ((so2, so, "store"), (wo2, wo, "wh"), (eo2, eo, "ech"), (r2, r, "reward")):
            assert a is None or torch.equal(a[..., :B], b_[..., :B]), (c.id, "in place", what)


def check_per_store_composition(h, c):
    """The one-store bodies composed the way the whole-horizon kernels compose a period (hostsim_env_step_*_per_store) against the
    quad composition, bit for bit, on an exact case without echelons - beyond the fixtures' three warehouses."""
    assert c.E == 0
    k, _ = reference(c)
    prob, s, w, e, ts, tw, te, dem, _keep = launch_inputs(k, "cpu", True)
    io = prob.make_io(s, w, None, dem, ts, tw, None)
    ld = prob.ldb
    fw = []
    for per_store in (False, True):
        so, wo, r = torch.zeros_like(s), torch.zeros_like(w), torch.zeros(ld)
        if per_store:
            assert h.hostsim_env_step_fwd_per_store(io, P(so), P(wo), P(r)) == 0
        else:
            h.hostsim_env_step_fwd(io, P(so), P(wo), None, P(r))
        fw.append((so, wo, r))
    for a, b_ in zip(*fw):
        assert torch.equal(a, b_), (c.id, "forward")
    gso, gwo = to_soa(k["g_out"]["store_inventories"], ld), to_soa(k["g_out"]["warehouse_inventories"], ld)
    grs = torch.zeros(ld)
    grs[:c.B] = k["g_reward"]
    bw = []
    for per_store in (False, True):
        gsi, gwi, gas, gaw = torch.zeros_like(s), torch.zeros_like(w), torch.zeros(c.S, prob.nsup, ld), torch.zeros(c.Wn, ld)
        tab = layout.Table(grs, 0, 1).t2()
        if per_store:
            assert h.hostsim_env_step_bwd_per_store(io, P(gso), P(gwo), tab, P(gsi), P(gwi), P(gas), P(gaw)) == 0
        else:
            h.hostsim_env_step_bwd(io, P(gso), P(gwo), None, tab, P(gsi), P(gwi), None, P(gas), P(gaw), None)
        bw.append((gsi, gwi, gas, gaw))
    for a, b_ in zip(*bw):
        assert torch.equal(a, b_), (c.id, "backward")
