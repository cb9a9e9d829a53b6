"""The glue kernels - segment sums, proportional allocations, the fused allocation + env step, the elementwise heads, the order
rounding - at their edges against float64, through the product library: the case tables and checkers of tests/glue_checks.py and
tests/kernel_checks.py on the HIP backend (tests/test_glue_checks_host.py shows on the CPU that the checkers notice each class of
kernel error), and the argument checks of the launchers."""
import pytest
import torch

import glue_checks as gc
import kernel_checks as kc
from neural_inventory_control_amd import _lib, layout

pytestmark = pytest.mark.gpu

ALL = [(name, c) for name, (cases, _) in gc.CHECKERS.items() for c in cases]


@pytest.fixture(scope="module")
def be():
    return gc.HipGlue()


@pytest.mark.parametrize("name,case", ALL, ids=[f"{n}-{c.id}" for n, c in ALL])
def test_glue_kernel_against_float64(be, name, case):
    gc.CHECKERS[name][1](be, case)      # (asserts, launch by launch, that nic_last_kernel() names the instantiation the case expects)


def test_every_launcher_cell_is_reached(be):
    """Every instantiation of every launcher of the glue kernels is named by nic_last_kernel() under some case: both segment-sum
    kernels <1> and <4>, gnn_alloc_env_{fwd,bwd}_kernel<4|8|16>, the allocations, the three heads, the rounding.  One case per cell
    is run here (again), so that the test stands on its own."""
    assert gc.expected_kernel_names() == gc.ALL_LAUNCHER_CELLS
    kc.RAN_KERNELS.clear()
    first = {}
    for c in gc.SEG_CASES + gc.TERMS_CASES:
        first.setdefault(gc.seg_expected_kernel(c), ("segment_sum_terms" if isinstance(c, gc.TermsCase) else "segment_sum", c))
    for c in gc.ALLOC_ENV_CASES:
        first.setdefault(gc.alloc_env_variant(c), ("alloc_env", c))
    for name in ("alloc", "groups", "round", "data_driven", "serial", "softplus"):
        first[name] = (name, gc.CHECKERS[name][0][0])
    for name, case in first.values():
        gc.CHECKERS[name][1](be, case)
    assert gc.ALL_LAUNCHER_CELLS <= kc.RAN_KERNELS, sorted(gc.ALL_LAUNCHER_CELLS - kc.RAN_KERNELS)


def test_report_the_referee_ratios():
    """(pytest -s) the worst max|kernel - fp64| / max|torch fp32 - fp64| per kernel and tensor of this session (DESIGN.md records them)"""
    for (backend, kernel, tensor), ratio in sorted(kc.REFEREE_FIGURES.items()):
        print(f"worst referee ratio  {backend:15s} {kernel:28s} {tensor:14s} {ratio:6.2f}")


# ---- argument checks: only arguments the host refuses before any launch ------------------------------------------------------------

def _refused(status, match):
    with pytest.raises(_lib.NicError, match=match):
        _lib.check(status)


def test_segment_sum_argument_checks_refuse_on_the_host():
    l, P, s = _lib.lib(), kc.P, _lib.current_stream()
    z = lambda *sh: torch.zeros(*sh, device="cuda")  # noqa: E731
    dst, src = z(2, 3, 32), z(2, 5, 32)
    off, it = torch.tensor([0, 1, 2, 3], dtype=torch.int32, device="cuda"), torch.tensor([0, 1, 2], dtype=torch.int32, device="cuda")
    for args in ((None, P(src), P(off), P(it)), (P(dst), None, P(off), P(it)), (P(dst), P(src), None, P(it)), (P(dst), P(src), P(off), None)):
        _refused(l.nic_segment_sum(args[0], 96, args[1], 160, args[2], args[3], None, 2, 3, 30, 32, 0, s), "null buffer")
    _refused(l.nic_segment_sum(P(dst), 96, P(src), 160, P(off), P(it), None, 2, 3, 33, 32, 0, s), "bad sizes")      # ldb < n_scenarios
    _refused(l.nic_segment_sum(P(dst), 96, P(src), 160, P(off), P(it), None, 0, 3, 30, 32, 0, s), "bad sizes")
    terms = (_lib.NicSegTerm * 5)()
    for t in terms:
        t.src, t.src_row_stride, t.offsets, t.items, t.scale = P(src), 160, P(off), P(it), None
    _refused(l.nic_segment_sum_terms(P(dst), 96, terms, 5, 2, 3, 30, 32, 0, s), "terms")      # more than NIC_SEG_MAX_TERMS
    _refused(l.nic_segment_sum_terms(P(dst), 96, terms, 0, 2, 3, 30, 32, 0, s), "terms")
    _refused(l.nic_segment_sum_terms(None, 96, terms, 2, 2, 3, 30, 32, 0, s), "terms")
    _refused(l.nic_segment_sum_terms(P(dst), 96, terms, 2, 2, 3, 33, 32, 0, s), "bad sizes")
    terms[1].items = None       # a segment term without its item list
    _refused(l.nic_segment_sum_terms(P(dst), 96, terms, 2, 2, 3, 30, 32, 0, s), "null term buffer")
    terms[1].items, terms[0].src = P(it), None
    _refused(l.nic_segment_sum_terms(P(dst), 96, terms, 2, 2, 3, 30, 32, 0, s), "null term buffer")
    torch.cuda.synchronize()


def test_allocation_argument_checks_refuse_on_the_host():
    l, P, s = _lib.lib(), kc.P, _lib.current_stream()
    z = lambda *sh: torch.zeros(*sh, device="cuda")  # noqa: E731
    S, E, ld, B = 3, 6, 32, 30
    out, oh, orders, sums, ratio, scale, g, d_out, g_oh = z(E, ld), z(ld), z(S + 1, ld), z(ld), z(ld), z(ld), z(S + 1, ld), z(E, ld), z(ld)
    fwd = [P(out), P(oh), P(orders), P(sums), P(ratio), P(scale)]
    for i in range(6):
        a = list(fwd)
        a[i] = None
        _refused(l.nic_gnn_alloc_fwd(*a, S, -1, 4, 1, B, ld, s), "null buffer")
    _refused(l.nic_gnn_alloc_fwd(*fwd, 0, -1, 4, 1, B, ld, s), "bad sizes")            # S = 0
    _refused(l.nic_gnn_alloc_fwd(*fwd, S, -1, 4, 1, 33, ld, s), "bad sizes")           # ldb < n_scenarios
    _refused(l.nic_gnn_alloc_fwd(*fwd, S, -1, -1, 1, B, ld, s), "bad sizes")           # no supplier edge
    bwd = [P(out), P(oh), P(g), P(sums), P(ratio), P(scale), P(d_out), P(g_oh)]
    for i in range(8):
        a = list(bwd)
        a[i] = None
        _refused(l.nic_gnn_alloc_bwd(*a, S, E, -1, 4, 1, B, ld, s), "null buffer")
    _refused(l.nic_gnn_alloc_bwd(*bwd, 0, E, -1, 4, 1, B, ld, s), "bad sizes")
    _refused(l.nic_gnn_alloc_bwd(*bwd, S, S, -1, 4, 1, B, ld, s), "bad sizes")         # n_edges <= S
    _refused(l.nic_gnn_alloc_bwd(*bwd, S, E, -1, 4, 1, 33, ld, s), "bad sizes")
    groups = torch.tensor([[0, 3, -1, 3]], dtype=torch.int32, device="cuda")
    order_row = torch.tensor([0, 1, 2, 3, -1, -1], dtype=torch.int32, device="cuda")
    gf = [P(out), P(oh), ld, P(orders), P(sums), P(ratio), P(scale), P(groups), P(order_row)]
    for i in (0, 1, 3, 4, 5, 6, 7, 8):
        a = list(gf)
        a[i] = None
        _refused(l.nic_gnn_alloc_groups_fwd(*a, 1, 1, B, ld, s), "null buffer")
    _refused(l.nic_gnn_alloc_groups_fwd(*gf, 0, 1, B, ld, s), "bad sizes")             # no group
    _refused(l.nic_gnn_alloc_groups_fwd(*gf, 1, 1, 33, ld, s), "bad sizes")
    gb = [P(out), P(oh), ld, P(g), P(sums), P(ratio), P(scale), P(d_out), P(g_oh), P(groups), P(order_row)]
    for i in (0, 1, 3, 4, 5, 6, 7, 8, 9, 10):
        a = list(gb)
        a[i] = None
        _refused(l.nic_gnn_alloc_groups_bwd(*a, 1, 4, 2, 1, B, ld, s), "null buffer")
    _refused(l.nic_gnn_alloc_groups_bwd(*gb, 1, 4, 2, 1, 33, ld, s), "bad sizes")
    _refused(l.nic_gnn_alloc_groups_bwd(*gb, 1, -1, 2, 1, B, ld, s), "bad sizes")
    _refused(l.nic_gnn_alloc_groups_bwd(*gb, 0, 4, 2, 1, B, ld, s), "bad sizes")
    torch.cuda.synchronize()


def test_fused_allocation_env_argument_checks_refuse_on_the_host(be):
    l, P, s = _lib.lib(), kc.P, _lib.current_stream()
    c = gc.ALLOC_ENV_CASES[1]
    p = gc.alloc_env_problem(c)
    k, dev, S = p["k"], "cuda", c.S
    prob = layout.EnvProblem(k["problem"], k["data"], dev)
    ld = prob.ldb
    st, w = layout.to_soa(k["state"]["store_inventories"].to(dev), ld), layout.to_soa(k["state"]["warehouse_inventories"].to(dev), ld)
    dem_t = k["data"]["demands"].to(dev)
    z = lambda *sh: torch.zeros(*sh, device=dev)  # noqa: E731
    out, orders, sums, ratio, scale, reward = z(p["n_edges"], ld), z(S + 1, ld), z(ld), z(ld), z(ld), z(ld)
    so, wo, d_out, g_orders = torch.zeros_like(st), torch.zeros_like(w), z(p["n_edges"], ld), z(S + 1, ld)
    gr = layout.Table(z(ld), 0, 1).t2()

    def io(**dims):
        ts, tw = gc.HipGlue._order_tables(orders, S, ld)
        x = prob.make_io(st, w, None, kc._demand_table(dem_t, 0), ts, tw, None)
        for n, v in dims.items():
            setattr(x.dims, n, v)
        return x

    def fwd(x, out_=out, e_sup=S):
        return l.nic_gnn_alloc_env_fwd(x, P(out_), P(orders), P(sums), P(ratio), P(scale), -1, e_sup, 1, P(so), P(wo), P(reward), s)

    def bwd(x, n_edges=p["n_edges"], d=d_out):
        return l.nic_gnn_alloc_env_bwd(x, P(out), P(sums), P(ratio), P(scale), n_edges, -1, S, 1, P(so), P(wo), gr, P(so), P(wo), P(g_orders),
                                       P(d), s)
    for call in (fwd, bwd):
        _refused(call(io(n_warehouses=2)), "one supplying warehouse")
        _refused(call(io(n_echelons=1)), "one supplying warehouse")
        for slots in (1, _lib.NIC_MAX_SLOTS + 1):
            _refused(call(io(store_slots=slots)), "pipeline lengths")
            _refused(call(io(warehouse_slots=slots)), "pipeline lengths")
        _refused(call(io(n_stores=0)), "bad sizes")
        _refused(call(io(ldb=c.B - 1)), "bad sizes")
        x = io()
        x.wh_inv = None
        _refused(call(x), "null buffer")
    _refused(fwd(io(), out_=None), "null buffer")
    _refused(fwd(io(), e_sup=-1), "null buffer / bad edge")
    x = io()
    x.store_orders.p = P(g_orders)      # order tables that are not the rows of `orders`
    _refused(fwd(x), "rows of `orders`")
    x = io()
    x.wh_orders.p = P(orders)
    _refused(fwd(x), "rows of `orders`")
    _refused(bwd(io(), n_edges=S), "bad edge count")      # n_edges <= S
    _refused(bwd(io(), d=None), "null buffer")
    torch.cuda.synchronize()


def test_head_and_rounding_argument_checks_refuse_on_the_host():
    l, P, s = _lib.lib(), kc.P, _lib.current_stream()
    z = lambda *sh: torch.zeros(*sh, device="cuda")  # noqa: E731
    S, Wn, Ww, ld, B = 3, 2, 2, 32, 30
    Z, wh, mask, so, wo, dZ, gwh = z(Wn + S * Wn, ld), z(Wn, Ww, ld), z(S, Wn), z(S * Wn, ld), z(Wn, ld), z(Wn + S * Wn, ld), z(Wn, Ww, ld)
    dd = [P(Z), P(wh), P(mask), P(so), P(wo)]
    for i in range(5):
        a = list(dd)
        a[i] = None
        _refused(l.nic_head_data_driven_fwd(*a, S, Wn, Ww, B, ld, s), "null buffer")
    _refused(l.nic_head_data_driven_fwd(*dd, 0, Wn, Ww, B, ld, s), "bad sizes")
    _refused(l.nic_head_data_driven_fwd(*dd, S, Wn, 0, B, ld, s), "bad sizes")
    _refused(l.nic_head_data_driven_fwd(*dd, S, Wn, Ww, 33, ld, s), "bad sizes")
    db = [P(Z), P(wh), P(mask), P(so), P(wo), P(dZ), P(gwh)]
    for i in range(7):
        a = list(db)
        a[i] = None
        _refused(l.nic_head_data_driven_bwd(*a, S, Wn, Ww, B, ld, s), "null buffer")
    _refused(l.nic_head_data_driven_bwd(*db, 0, Wn, Ww, B, ld, s), "bad sizes")
    _refused(l.nic_head_data_driven_bwd(*db, S, Wn, Ww, 33, ld, s), "bad sizes")
    E, We = 1, 2
    Zs, w1, ech, o1, eo = z(E + 2, ld), z(1, Ww, ld), z(E, We, ld), z(1, ld), z(E, ld)
    sf = [P(Zs), P(w1), P(ech), 20.0, P(o1), P(o1), P(eo)]
    for i in (0, 1, 2, 4, 5, 6):
        a = list(sf)
        a[i] = None
        _refused(l.nic_head_serial_fwd(*a, E, Ww, We, B, ld, s), "null buffer")
    _refused(l.nic_head_serial_fwd(*sf, -1, Ww, We, B, ld, s), "bad sizes")
    _refused(l.nic_head_serial_fwd(*sf, E, Ww, We, 33, ld, s), "bad sizes")
    sb = [P(Zs), P(w1), P(ech), 20.0, P(o1), P(o1), P(eo), P(Zs), P(w1), P(ech)]
    for i in (0, 1, 2, 4, 5, 6, 7, 8, 9):
        a = list(sb)
        a[i] = None
        _refused(l.nic_head_serial_bwd(*a, E, Ww, We, B, ld, s), "null buffer")
    _refused(l.nic_head_serial_bwd(*sb, E, Ww, We, 33, ld, s), "bad sizes")
    _refused(l.nic_head_softplus_fwd(None, P(o1), 1, B, ld, s), "bad arguments")
    _refused(l.nic_head_softplus_fwd(P(o1), None, 1, B, ld, s), "bad arguments")
    _refused(l.nic_head_softplus_fwd(P(o1), P(eo), 0, B, ld, s), "bad arguments")
    _refused(l.nic_head_softplus_fwd(P(o1), P(eo), 1, 33, ld, s), "bad arguments")
    _refused(l.nic_head_softplus_bwd(P(o1), P(eo), None, 1, B, ld, s), "bad arguments")
    _refused(l.nic_head_softplus_bwd(P(o1), P(eo), P(eo), 1, 33, ld, s), "bad arguments")
    _refused(l.nic_round_orders(None, 1, B, ld, s), "bad arguments")
    _refused(l.nic_round_orders(P(o1), 0, B, ld, s), "bad arguments")
    _refused(l.nic_round_orders(P(o1), 1, 33, ld, s), "bad arguments")
    torch.cuda.synchronize()
