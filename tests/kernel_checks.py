"""Backend-agnostic parity checks of the kernel arithmetic.

The same checks run against two builds of the same NIC_HD bodies:
  * HostSimBackend — tests/hostsim (g++), CPU tensors, runs on the CPU container (`-m "not gpu"`);
  * HipBackend     — the product library libnic_hip.so through the C ABI, device tensors (`-m gpu`).
Expected values come from the golden fixtures (reference outputs) and the oracle's autograd.
"""
import torch
import torch.nn.functional as F

from golden_io import Golden, ZERO_LEAD_CASES
from neural_inventory_control_amd import _lib, layout
from neural_inventory_control_amd.layout import EnvProblem, Table, pad_ld, ref_view, to_soa
from oracle import inventory_oracle as orc

P = lambda x: x.data_ptr() if x is not None else None  # noqa: E731


class HostSimBackend:
    device = "cpu"

    def __init__(self):
        import hostsim_util
        self.h = hostsim_util.load()

    def sync(self):
        pass

    def env_fwd(self, io, so, wo, eo, r):
        self.h.hostsim_env_step_fwd(io, P(so), P(wo), P(eo), P(r))

    def env_bwd(self, io, gso, gwo, geo, gr, gsi, gwi, gei, gas, gaw, gae):
        self.h.hostsim_env_step_bwd(io, P(gso), P(gwo), P(geo), gr, P(gsi), P(gwi), P(gei), P(gas), P(gaw), P(gae))

    def head_warehouse_fwd(self, Z, wh, adj, ub, trans, so, wo, S, Wn, Ww, B, ldb):
        self.h.hostsim_head_warehouse_fwd(P(Z), P(wh), P(adj), ub, trans, P(so), P(wo), S, Wn, Ww, B, ldb)

    def head_warehouse_bwd(self, Z, wh, adj, ub, trans, gso, gwo, dZ, gwi, S, Wn, Ww, B, ldb):
        self.h.hostsim_head_warehouse_bwd(P(Z), P(wh), P(adj), ub, trans, P(gso), P(gwo), P(dZ), P(gwi), S, Wn, Ww, B, ldb)

    def head_softplus_fwd(self, Z, o, rows, B, ldb):
        self.h.hostsim_head_softplus_fwd(P(Z), P(o), rows, B, ldb)

    def head_softplus_bwd(self, Z, g, dZ, rows, B, ldb):
        self.h.hostsim_head_softplus_bwd(P(Z), P(g), P(dZ), rows, B, ldb)

    def head_serial_fwd(self, Z, wh, ech, ub, so, wo, eo, E, Ww, We, B, ldb):
        self.h.hostsim_head_serial_fwd(P(Z), P(wh), P(ech), ub, P(so), P(wo), P(eo), E, Ww, We, B, ldb)

    def head_serial_bwd(self, Z, wh, ech, ub, gso, gwo, geo, dZ, gwi, gei, E, Ww, We, B, ldb):
        self.h.hostsim_head_serial_bwd(P(Z), P(wh), P(ech), ub, P(gso), P(gwo), P(geo), P(dZ), P(gwi), P(gei), E, Ww, We, B, ldb)


class HipBackend:
    device = "cuda"

    def __init__(self):
        _lib.require_device()
        self.l = _lib.lib()

    def sync(self):
        torch.cuda.synchronize()

    @staticmethod
    def _s():
        return _lib.current_stream()

    def env_fwd(self, io, so, wo, eo, r, zero_lead_upstream=0):
        _lib.check(self.l.nic_env_step_fwd(io, P(so), P(wo), P(eo), P(r), zero_lead_upstream, self._s()))

    def env_bwd(self, io, gso, gwo, geo, gr, gsi, gwi, gei, gas, gaw, gae, zero_lead_upstream=0):
        _lib.check(self.l.nic_env_step_bwd(io, P(gso), P(gwo), P(geo), gr, P(gsi), P(gwi), P(gei), P(gas), P(gaw), P(gae),
                                           zero_lead_upstream, self._s()))

    def head_warehouse_fwd(self, Z, wh, adj, ub, trans, so, wo, S, Wn, Ww, B, ldb):
        _lib.check(self.l.nic_head_warehouse_fwd(P(Z), P(wh), P(adj), ub, trans, P(so), P(wo), S, Wn, Ww, B, ldb, self._s()))

    def head_warehouse_bwd(self, Z, wh, adj, ub, trans, gso, gwo, dZ, gwi, S, Wn, Ww, B, ldb):
        _lib.check(self.l.nic_head_warehouse_bwd(P(Z), P(wh), P(adj), ub, trans, P(gso), P(gwo), P(dZ), P(gwi), S, Wn, Ww,
                                                 B, ldb, self._s()))

    def head_softplus_fwd(self, Z, o, rows, B, ldb):
        _lib.check(self.l.nic_head_softplus_fwd(P(Z), P(o), rows, B, ldb, self._s()))

    def head_softplus_bwd(self, Z, g, dZ, rows, B, ldb):
        _lib.check(self.l.nic_head_softplus_bwd(P(Z), P(g), P(dZ), rows, B, ldb, self._s()))

    def head_serial_fwd(self, Z, wh, ech, ub, so, wo, eo, E, Ww, We, B, ldb):
        _lib.check(self.l.nic_head_serial_fwd(P(Z), P(wh), P(ech), ub, P(so), P(wo), P(eo), E, Ww, We, B, ldb, self._s()))

    def head_serial_bwd(self, Z, wh, ech, ub, gso, gwo, geo, dZ, gwi, gei, E, Ww, We, B, ldb):
        _lib.check(self.l.nic_head_serial_bwd(P(Z), P(wh), P(ech), ub, P(gso), P(gwo), P(geo), P(dZ), P(gwi), P(gei), E, Ww,
                                              We, B, ldb, self._s()))


# ------------------------------------------------------------------------------------------------------------------

def _state_soa(st, prob, dev):
    s = to_soa(st["store_inventories"].to(dev), prob.ldb)
    w = to_soa(st["warehouse_inventories"].to(dev), prob.ldb) if prob.Wn else None
    e = to_soa(st["echelon_inventories"].to(dev), prob.ldb) if prob.E else None
    return s, w, e


def _orders_tables(act, dev):
    """Orders exactly as a reference-style policy hands them over: (B,S,Wn) scenario-major tensors."""
    a = {k: v.to(dev) for k, v in act.items()}
    keep = list(a.values())
    return (Table.from_orders(a["stores"]),
            Table.from_orders(a["warehouses"][:, :, 0]) if "warehouses" in a else None,
            Table.from_orders(a["echelons"][:, :, 0]) if "echelons" in a else None, keep)


def _demand_table(demands_dev, t):
    d = demands_dev
    return Table(d[:, :, t], d.stride(1), d.stride(0))


def knife_edge_scenarios(st, act):
    """Scenarios whose warehouse on-hand after shipping (environment.py:249) is within float noise of 0 WITHOUT being
    structurally 0: the `>= 0` mask of clamp's backward then depends on the summation order of `sum(dim=1)`, which no
    two implementations share (the reference's own CPU and GPU paths differ there too).  Excluded from gradient
    comparisons; exact zeros (structural ties) stay in."""
    B = st["store_inventories"].shape[0]
    bad = torch.zeros(B, dtype=torch.bool)
    if "warehouse_inventories" in st:
        orders = act["stores"].detach().double()
        after = st["warehouse_inventories"].detach()[:, :, 0].double() - orders.sum(dim=1)
        scale = orders.abs().sum(dim=1) + 1e-30
        bad |= ((after.abs() / scale < 1e-6) & ((orders != 0).sum(dim=1) >= 2)).any(dim=1)  # >= 2 addends: order matters
    return bad


def check_env_forward(be, name):
    g = Golden(name)
    c = g.fresh_config()
    data = g.data
    dev = be.device
    prob = EnvProblem(c["problem_params"], data, dev)
    B, T = c["n"], c["periods"]
    rewards = g.tensor("rewards")
    demands = data["demands"].to(dev)
    shift = c["observation_params"]["demand"]["period_shift"]  # real-data settings start inside the trace (environment.py:177)
    # the quantile policies' orders are float64 upstream (float64 probability points, quantile_forecaster.py:33), and with them
    # the reference's state from the first step on: the float32 kernel is then compared to rounding, not bit for bit
    f64 = g.states(1)["store_inventories"].dtype == torch.float64
    for t in range(T):
        s, w, e = _state_soa({k: v.float() for k, v in g.states(t).items()}, prob, dev)
        ts, tw, te, _keep = _orders_tables({k: v.float() for k, v in g.actions(t).items()}, dev)
        dem_t = _demand_table(demands, t + shift)   # (kept alive: the io holds raw addresses)
        io = prob.make_io(s, w, e, dem_t, ts, tw, te)
        so = torch.zeros_like(s)
        wo = torch.zeros_like(w) if w is not None else None
        eo = torch.zeros_like(e) if e is not None else None
        r = torch.zeros(prob.ldb, device=dev)
        be.env_fwd(io, so, wo, eo, r)
        be.sync()
        nxt = g.states(t + 1)
        want_r = rewards[t].float()
        if name in ZERO_LEAD_CASES:   # one oracle step from the fixture's state with zero-lead orders dropped (see golden_io)
            env = orc.env_reset(T, c["problem_params"], data, c["observation_params"])
            env.obs.update({k: v.float().clone() for k, v in g.states(t).items()})
            env.t, env.zero_lead_orders = t, "drop"
            want_r = orc.env_step(env, {k: v.float() for k, v in g.actions(t).items()})
            nxt = {k: v for k, v in env.obs.items() if k.endswith("inventories")}
        # integer slot placement and the store pipelines are exact; sums over stores may differ in the last bit
        if f64:
            torch.testing.assert_close(ref_view(so, B).cpu(), nxt["store_inventories"].float(), rtol=2e-6, atol=1e-4)
        else:
            assert torch.equal(ref_view(so, B).cpu(), nxt["store_inventories"]), (t, "stores")
        if prob.Wn:
            torch.testing.assert_close(ref_view(wo, B).cpu(), nxt["warehouse_inventories"], rtol=2e-6, atol=1e-5)
        if prob.E:
            torch.testing.assert_close(ref_view(eo, B).cpu(), nxt["echelon_inventories"], rtol=2e-6, atol=1e-5)
        torch.testing.assert_close(r[:B].cpu(), want_r, rtol=2e-6, atol=1e-3 if f64 else 1e-5)
        assert float(r[B:].abs().sum()) == 0.0


# ---- zero-lead orders: a hand-computed period (pins the "drop" semantics ZERO_LEAD_CASES are compared against) ----------------
def zero_lead_micro_case():
    """One period, one scenario, 2 stores x 2 warehouses, pipelines of 3 slots, lost demand; store 0 is connected to warehouse 1
    only (lead time 0 on warehouse 0) and still carries an order of 4 in warehouse 0's column - the situation upstream's GNN
    creates on the shipped many-warehouse adjacency (neural_networks.py:1423-1428).  Expected values are worked out BY HAND below
    for the semantics the HIP env step implements ("drop": the order reaches no pipeline slot, but it still leaves warehouse 0 -
    the outflow sum has no filter, environment.py:247):

      store 0: on hand 5, demand 3 -> after 2: cost 1 * 2 = 2;   shift [2 + 1, 0, 0]; order 4 @ lead 0: dropped; 1.5 @ lead 2 -> slot 1
               -> [3, 1.5, 0]
      store 1: on hand 2, demand 4 -> after -2: cost 8 * 2 = 16, lost demand -> 0; shift [0 + 0, 3, 0]; 2 @ lead 3 -> slot 2,
               0.5 @ lead 1 -> slot 0                      -> [0.5, 3, 2]
      wh 0: on hand 10, ships 4 + 2 = 6 -> after 4: holding 0.25 * 4 = 1, edge 0.5 * 7 = 3.5; shift [4 + 0, 1, 0]; 7 @ lead 3 -> [4, 1, 7]
      wh 1: on hand 1, ships 1.5 + 0.5 = 2 -> after -1: holding 0, edge 1.5 * 3 = 4.5;      shift [-1 + 2, 0, 0]; 3 @ lead 3 -> [1, 0, 3]
      cost of the period = 2 + 16 + (1 + 3.5) + (0 + 4.5) = 27
    """
    t = torch.tensor
    problem = {"n_stores": 2, "n_warehouses": 2, "n_extra_echelons": 0, "lost_demand": True, "maximize_profit": False,
               "warehouse_store_adjacency": [[0, 1], [1, 1]]}
    data = {"demands": t([[[3.0], [4.0]]]), "initial_inventories": t([[[5.0, 1.0, 0.0], [2.0, 0.0, 3.0]]]),
            "underage_costs": t([[10.0, 8.0]]), "holding_costs": t([[1.0, 2.0]]),
            "lead_times": t([[[0.0, 2.0], [3.0, 1.0]]]),
            "initial_warehouse_inventories": t([[[10.0, 0.0, 1.0], [1.0, 2.0, 0.0]]]),
            "warehouse_holding_costs": t([[0.25, 0.5]]), "warehouse_lead_times": t([[3.0, 3.0]]),
            "warehouse_edge_costs": t([[0.5, 1.5]])}
    action = {"stores": t([[[4.0, 1.5], [2.0, 0.5]]]), "warehouses": t([[[7.0], [3.0]]])}
    want = {"store_inventories": t([[[3.0, 1.5, 0.0], [0.5, 3.0, 2.0]]]),
            "warehouse_inventories": t([[[4.0, 1.0, 7.0], [1.0, 0.0, 3.0]]]), "reward": t([27.0])}
    obs_params = {"include_warehouse_inventory": True, "include_static_features": {"holding_costs": True, "underage_costs": True,
                                                                                  "lead_times": True},
                  "demand": {"past_periods": 0, "period_shift": 0}, "include_days_to_christmas": False,
                  "time_features": None, "sample_features": None}
    return problem, data, action, want, obs_params


def check_zero_lead_micro(be):
    """The kernel (host build or HIP) and the oracle's drop mode against the hand-computed numbers; the oracle's default mode
    (upstream's flat-index `put`) differs: it books the dropped 4 on the element in front of store 0's pipeline."""
    problem, data, action, want, obs_params = zero_lead_micro_case()
    for mode in ("drop", "upstream"):
        env = orc.env_reset(1, problem, data, obs_params)
        env.zero_lead_orders = mode
        r = orc.env_step(env, action)
        if mode == "drop":
            assert torch.equal(env.obs["store_inventories"], want["store_inventories"])
            assert torch.equal(env.obs["warehouse_inventories"], want["warehouse_inventories"])
            assert torch.equal(r, want["reward"])
        else:   # one scenario: the misplaced order wraps to the LAST element of the batch (store 1's last slot)
            leak = want["store_inventories"].clone()
            leak[0, 1, 2] += 4.0
            assert torch.equal(env.obs["store_inventories"], leak)
    dev = be.device
    prob = EnvProblem(problem, data, dev)
    s, w, _ = _state_soa({"store_inventories": data["initial_inventories"], "warehouse_inventories": data["initial_warehouse_inventories"]},
                         prob, dev)
    ts, tw, te, _keep = _orders_tables(action, dev)
    dem = data["demands"].to(dev)   # (kept alive: the table below only holds its address)
    io = prob.make_io(s, w, None, _demand_table(dem, 0), ts, tw, te)
    so, wo, r = torch.zeros_like(s), torch.zeros_like(w), torch.zeros(prob.ldb, device=dev)
    be.env_fwd(io, so, wo, None, r)
    be.sync()
    assert torch.equal(ref_view(so, 1).cpu(), want["store_inventories"])
    assert torch.equal(ref_view(wo, 1).cpu(), want["warehouse_inventories"])
    assert torch.equal(r[:1].cpu(), want["reward"])
    if isinstance(be, HipBackend):   # the HIP entry point's own upstream mode (round 6): the oracle's default numbers, same launch
        so2, wo2, r2 = torch.zeros_like(s), torch.zeros_like(w), torch.zeros(prob.ldb, device=dev)
        be.env_fwd(io, so2, wo2, None, r2, zero_lead_upstream=1)
        be.sync()
        leak = want["store_inventories"].clone()
        leak[0, 1, 2] += 4.0
        assert torch.equal(ref_view(so2, 1).cpu(), leak)
        assert torch.equal(wo2, wo) and torch.equal(r2, r)


def check_env_backward(be, name, profit):
    g = Golden(name)
    c = g.fresh_config()
    c["problem_params"]["maximize_profit"] = profit
    data = g.data
    dev = be.device
    prob = EnvProblem(c["problem_params"], data, dev)
    B = c["n"]
    demands = data["demands"].to(dev)
    gen = torch.Generator().manual_seed(7)
    compared = 0
    shift = c["observation_params"]["demand"]["period_shift"]
    for t in (0, 1, c["periods"] // 2, c["periods"] - 1):
        st = {k: v.float().clone().requires_grad_(True) for k, v in g.states(t).items()}
        act = {k: v.float().clone().requires_grad_(True) for k, v in g.actions(t).items()}
        with torch.no_grad():  # force exact ties / zeros: on-hand == demand, zero orders
            st["store_inventories"][0, :, 0] = data["demands"][0, :, t + shift]
            act["stores"][1 % B] = 0.0
        env = orc.env_reset(c["periods"], c["problem_params"], data, c["observation_params"])
        env.obs.update(st)
        env.t = t
        env.zero_lead_orders = "drop" if name in ZERO_LEAD_CASES else "upstream"
        reward = orc.env_step(env, act)
        keys = [k for k in ("store_inventories", "warehouse_inventories", "echelon_inventories") if k in st]
        g_out = {k: torch.randn(env.obs[k].shape, generator=gen) for k in keys}
        g_r = torch.randn(B, generator=gen)
        ((reward * g_r).sum() + sum((env.obs[k] * g_out[k]).sum() for k in keys)).backward()
        for leaf in list(st.values()) + list(act.values()):
            if leaf.grad is None:  # e.g. every order is 0 -> the reference skips the put entirely (environment.py:427)
                leaf.grad = torch.zeros_like(leaf)

        s, w, e = _state_soa({k: v.detach() for k, v in st.items()}, prob, dev)
        ts, tw, te, _keep = _orders_tables({k: v.detach() for k, v in act.items()}, dev)
        dem_t = _demand_table(demands, t + shift)   # (kept alive: the io holds raw addresses)
        io = prob.make_io(s, w, e, dem_t, ts, tw, te)
        gso = to_soa(g_out["store_inventories"].to(dev), prob.ldb)
        gwo = to_soa(g_out["warehouse_inventories"].to(dev), prob.ldb) if prob.Wn else None
        geo = to_soa(g_out["echelon_inventories"].to(dev), prob.ldb) if prob.E else None
        grs = torch.zeros(prob.ldb, device=dev)
        grs[:B] = g_r.to(dev)
        gsi = torch.zeros_like(s)
        gwi = torch.zeros_like(w) if prob.Wn else None
        gei = torch.zeros_like(e) if prob.E else None
        gas = torch.zeros(prob.S, prob.nsup, prob.ldb, device=dev)
        gaw = torch.zeros(prob.Wn, prob.ldb, device=dev) if prob.Wn else None
        gae = torch.zeros(prob.E, prob.ldb, device=dev) if prob.E else None
        be.env_bwd(io, gso, gwo, geo, layout.Table(grs, 0, 1).t2(), gsi, gwi, gei, gas, gaw, gae)
        be.sync()
        tol = dict(rtol=1e-5, atol=1e-5)
        ok = ~knife_edge_scenarios(st, act)
        compared += int(ok.sum())
        torch.testing.assert_close(ref_view(gsi, B).cpu()[ok], st["store_inventories"].grad[ok], **tol)
        torch.testing.assert_close(ref_view(gas, B).cpu()[ok], act["stores"].grad[ok], **tol)
        if prob.Wn:
            torch.testing.assert_close(ref_view(gwi, B).cpu()[ok], st["warehouse_inventories"].grad[ok], **tol)
            torch.testing.assert_close(ref_view(gaw, B).cpu()[ok], act["warehouses"].grad[:, :, 0][ok], **tol)
        if prob.E:
            torch.testing.assert_close(ref_view(gei, B).cpu()[ok], st["echelon_inventories"].grad[ok], **tol)
            torch.testing.assert_close(ref_view(gae, B).cpu()[ok], act["echelons"].grad[:, :, 0][ok], **tol)
    assert compared >= 2 * B  # saturated softmax heads put many late-period scenarios on the knife edge


# The fp64 referee of the warehouse head (the cases of WAREHOUSE_HEAD_REFEREE_CASES).  The fixed band of the first cases
# (rtol 3e-5, atol 3e-6 against the float32 torch expression) sits at the noise of that float32 reference once a softmax runs over
# 17+ stores: the host build missed it by one element of ~7,000 at (S, Wn) = (21, 9) and (17, 12).  So both are judged against
# the SAME expression in float64, per output tensor:
#     max|kernel - fp64|  <=  c * max|torch fp32 - fp64|  +  one ulp of the tensor's largest magnitude
# c = twice the worst ratio max|kernel - fp64| / max|torch fp32 - fp64| measured over the referee cases, both transshipment
# modes, all four tensors, per path (the check prints every figure before it asserts: pytest -s).  Measured:
#                          host build (expf, division)      HIP (v_exp_f32, e * v_rcp_f32)
#   quad path (S <= 64)    <= 1.58 (allocations, S 64 Wn 17)   <= 1.58 (the same element)
#   one-lane path (S > 64) 3.43 allocations, 8.16 g_wh_inv     3.43 allocations, 8.16 g_wh_inv   (S 70: 70 serial float32 adds)
# (warehouse orders and dZ sit at 1.00 on both: their largest errors are the sigmoid row's, the same arithmetic as torch's.)
# c = 2 x 1.58 and 2 x 8.16, rounded up to two digits.
HEAD_REFEREE_C = {"quad": 3.2, "wide": 16.4}


def _ulp(x):
    """spacing of float32 at magnitude x"""
    return float(torch.nextafter(torch.tensor(float(x), dtype=torch.float32), torch.tensor(float("inf"))) - float(x))


def _head_expression(Z, wh, adj_t, ub, trans, g_so, g_wo, dtype):
    """oracle arithmetic of neural_networks.py:393-426 on given logits + autograd, in `dtype`"""
    Z = Z.detach().to(dtype).requires_grad_(True)
    wh = wh.detach().to(dtype).requires_grad_(True)
    Wn, S = adj_t.shape
    store_logits = Z[:, :S * Wn].view(-1, S, Wn)
    alloc = torch.zeros_like(store_logits)
    for w in range(Wn):
        conn = adj_t[w].nonzero(as_tuple=True)[0]
        if len(conn) > 0:
            alloc[:, conn, w] = orc._softmax_share_of_stock(store_logits[:, conn, w], wh[:, w:w + 1], trans)
    wh_orders = torch.sigmoid(Z[:, S * Wn:]) * torch.tensor([ub], dtype=dtype)
    ((alloc * g_so.to(dtype)).sum() + (wh_orders * g_wo.to(dtype)).sum()).backward()
    return alloc.detach(), wh_orders.detach(), Z.grad, wh.grad


def check_warehouse_head(be, S, Wn, adj, trans, B=37, referee=False):
    """referee=False: the fixed bands against the float32 expression (the first cases, unchanged).  referee=True: the fp64 referee
    described at HEAD_REFEREE_C; returns the measured ratios {tensor: max|kernel - fp64| / max|torch fp32 - fp64|}."""
    dev = be.device
    Ww = 3
    ldb = pad_ld(B)
    gen = torch.Generator().manual_seed(3)
    Z = (torch.randn(B, S * Wn + Wn, generator=gen) * 3)
    wh = (torch.rand(B, Wn, Ww, generator=gen) * 20)
    wh[0, :, 0] = 0.0  # empty warehouse
    ub = 123.5
    adj_t = torch.ones(1, S) if Wn == 1 else torch.tensor(adj, dtype=torch.float32)
    g_so = torch.randn(B, S, Wn, generator=gen)
    g_wo = torch.randn(B, Wn, generator=gen)
    alloc, wh_orders, Z_grad, wh_grad = _head_expression(Z, wh, adj_t, ub, trans, g_so, g_wo, torch.float32)

    Zs, whs = to_soa(Z.to(dev), ldb), to_soa(wh.to(dev), ldb)
    adj_i = adj_t.to(torch.int32).contiguous().to(dev)
    so, wo = torch.zeros(S, Wn, ldb, device=dev), torch.zeros(Wn, ldb, device=dev)
    be.head_warehouse_fwd(Zs, whs, adj_i, ub, int(trans), so, wo, S, Wn, Ww, B, ldb)
    be.sync()
    dZ = torch.zeros(S * Wn + Wn, ldb, device=dev)
    gwi = torch.zeros(Wn, Ww, ldb, device=dev)
    gso_s, gwo_s = to_soa(g_so.to(dev), ldb), to_soa(g_wo.to(dev), ldb)
    be.head_warehouse_bwd(Zs, whs, adj_i, ub, int(trans), gso_s, gwo_s, dZ, gwi, S, Wn, Ww, B, ldb)
    be.sync()
    # structurally-zero orders must be EXACT zeros (the env's `!= 0` filter depends on it)
    assert torch.equal(ref_view(so, B).cpu() == 0, alloc == 0)
    got = {"allocations": ref_view(so, B).cpu(), "warehouse_orders": ref_view(wo, B).cpu(), "dZ": ref_view(dZ, B).cpu(),
           "g_wh_inv": ref_view(gwi, B).cpu()}
    if not referee:
        torch.testing.assert_close(got["allocations"], alloc, rtol=3e-6, atol=1e-6)
        torch.testing.assert_close(got["warehouse_orders"], wh_orders, rtol=3e-6, atol=1e-6)
        torch.testing.assert_close(got["dZ"], Z_grad, rtol=3e-5, atol=3e-6)
        torch.testing.assert_close(got["g_wh_inv"], wh_grad, rtol=3e-5, atol=3e-6)
        return None
    ref32 = dict(zip(got, (alloc, wh_orders, Z_grad, wh_grad)))
    ref64 = dict(zip(got, _head_expression(Z, wh, adj_t, ub, trans, g_so, g_wo, torch.float64)))
    c = HEAD_REFEREE_C["quad" if S <= 64 else "wide"]
    ratios, bad = {}, []
    for name in got:
        err_k = float((got[name].double() - ref64[name]).abs().max())
        err_t = float((ref32[name].double() - ref64[name]).abs().max())
        ulp = _ulp(ref64[name].abs().max())
        ratios[name] = err_k / err_t if err_t > 0 else (0.0 if err_k == 0 else float("inf"))
        print(f"head referee S={S} Wn={Wn} trans={int(trans)} {type(be).__name__} {name}: kernel {err_k:.3e} torch32 {err_t:.3e} "
              f"ratio {ratios[name]:.2f} ulp {ulp:.1e}")
        if not err_k <= c * err_t + ulp:
            bad.append((name, err_k, err_t, ulp))
    assert not bad, (S, Wn, trans, c, bad)
    return ratios


def check_softplus_head(be):
    dev = be.device
    B, ldb = 50, 64
    Z = torch.linspace(-30, 30, B).reshape(B, 1).clone().requires_grad_(True)
    y = F.softplus(Z + 1)
    g = torch.randn(B, 1)
    (y * g).sum().backward()
    out, dZ = torch.zeros(1, ldb, device=dev), torch.zeros(1, ldb, device=dev)
    Zs, gs = to_soa(Z.detach().to(dev), ldb), to_soa(g.to(dev), ldb)
    be.head_softplus_fwd(Zs, out, 1, B, ldb)
    be.head_softplus_bwd(Zs, gs, dZ, 1, B, ldb)
    be.sync()
    torch.testing.assert_close(ref_view(out, B).cpu(), y.detach(), rtol=3e-6, atol=1e-7)
    torch.testing.assert_close(ref_view(dZ, B).cpu(), Z.grad, rtol=3e-6, atol=1e-7)


def check_serial_head(be, E):
    dev = be.device
    B, Ww, We = 41, 3, 4
    ldb = pad_ld(B)
    gen = torch.Generator().manual_seed(5)
    Z = torch.randn(B, E + 2, generator=gen).requires_grad_(True)
    wh = (torch.rand(B, 1, Ww, generator=gen) * 9).requires_grad_(True)
    ech = (torch.rand(B, E, We, generator=gen) * 9).requires_grad_(True)
    ub = 20.0
    upstream = torch.concat((torch.tensor([ub]).unsqueeze(1).expand(B, -1), ech[:, :, 0], wh[:, :, 0]), dim=1)
    alloc = torch.sigmoid(Z) * upstream  # neural_networks.py:335-344
    g = torch.randn(B, E + 2, generator=gen)
    (alloc * g).sum().backward()
    Zs, whs, echs = (to_soa(x.detach().to(dev), ldb) for x in (Z, wh, ech))
    so, wo, eo = torch.zeros(1, 1, ldb, device=dev), torch.zeros(1, ldb, device=dev), torch.zeros(E, ldb, device=dev)
    be.head_serial_fwd(Zs, whs, echs, ub, so, wo, eo, E, Ww, We, B, ldb)
    be.sync()
    torch.testing.assert_close(ref_view(eo, B).cpu(), alloc.detach()[:, :E], rtol=3e-6, atol=1e-7)
    torch.testing.assert_close(wo[0, :B].cpu(), alloc.detach()[:, E], rtol=3e-6, atol=1e-7)
    torch.testing.assert_close(so[0, 0, :B].cpu(), alloc.detach()[:, E + 1], rtol=3e-6, atol=1e-7)
    dZ, gwi, gei = (torch.zeros(E + 2, ldb, device=dev), torch.zeros(1, Ww, ldb, device=dev),
                    torch.zeros(E, We, ldb, device=dev))
    gs = to_soa(g.to(dev), ldb)
    g_store, g_wh, g_ech = gs[E + 1:], gs[E:E + 1], gs[:E]
    be.head_serial_bwd(Zs, whs, echs, ub, g_store, g_wh, g_ech, dZ, gwi, gei, E, Ww, We, B, ldb)
    be.sync()
    torch.testing.assert_close(ref_view(dZ, B).cpu(), Z.grad, rtol=3e-5, atol=1e-6)
    torch.testing.assert_close(ref_view(gwi, B).cpu(), wh.grad, rtol=3e-5, atol=1e-6)
    torch.testing.assert_close(ref_view(gei, B).cpu(), ech.grad, rtol=3e-5, atol=1e-6)


def _cfg5_adjacency():
    from cases import CASES
    return CASES["cfg5_many_warehouses_3x64_vanilla"]["problem_overrides"]["warehouse_store_adjacency"]


WAREHOUSE_HEAD_CASES = [
    (64, 3, _cfg5_adjacency()),  # BASELINE cfg5's real topology: 16 stores per lane of the quad, 195 logit rows
    (16, 1, None),
    (10, 2, [[0, 0, 1, 1, 1, 0, 1, 1, 1, 0], [1, 1, 1, 1, 1, 1, 0, 1, 1, 1]]),
    (8, 3, [[1, 1, 0, 0, 1, 0, 1, 0], [0, 1, 1, 1, 0, 0, 1, 1], [1, 0, 0, 1, 0, 1, 0, 1]]),
    (4, 2, [[1, 1, 1, 1], [0, 0, 0, 0]]),  # a warehouse without any connected store
]


def _referee_adjacency(S, Wn):
    """fixed seed; warehouse 0 serves every store, warehouse 1 a single one, warehouse 2 (if there is one) none"""
    gen = torch.Generator().manual_seed(1000 * S + Wn)
    adj = (torch.rand(Wn, S, generator=gen) < 0.6).int()
    adj[0] = 1
    if Wn > 1:
        adj[1] = 0
        adj[1, S // 2] = 1
    if Wn > 2:
        adj[2] = 0
    return adj.tolist()


# The dispatch points of nic_head_warehouse_* the first cases never reach (B = 150: three scenario workgroups, the last ragged):
# grid.y = min(Wn, 8) workgroups striding over warehouses (9, 12, 17, 32), the sq = 8 variant (17 <= S <= 32), the one-lane kernel
# for S > 64 with its grid.y = min(Wn, 4), a single store.
WAREHOUSE_HEAD_REFEREE_B = 150
WAREHOUSE_HEAD_REFEREE_CASES = [(S, Wn, _referee_adjacency(S, Wn)) for S, Wn in
                                ((21, 9), (17, 12), (32, 4), (5, 32), (64, 17), (70, 2), (1, 5))]
