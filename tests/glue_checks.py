"""The small kernels between the big ones - segment sums, proportional allocations, the fused allocation + env step, the order
rounding - at their edges, against float64 ("Glue kernels at their edges").

Fixed case tables, input builders, float64 references and checkers that take a backend, like mlp3_checks.py and env_exact_cases.py:
  * HipGlue   - the product library through the C ABI / ops on the device (tests/test_gpu_glue_kernels.py);
  * TorchGlue - a float32 restatement of every kernel in aten ops on the CPU, with a `defect=` switch that restates one class of
                kernel error each (tests/test_glue_checks_host.py: the clean restatement passes every case, every defect fails at
                least one - the proof that the checkers would notice, without ever running a broken kernel on a device).
The checks of the three NIC_HD heads (data_driven, serial, softplus) live in kernel_checks.py, so that the host build of their
bodies runs them too; TorchGlue implements those entry points as well (for the defects that concern them).

The two input families, the referee bound and the helpers shared with the heads are described in kernel_checks.py.  Nothing is
drawn at run time beyond fixed seeds; no scenario is excluded anywhere; the only tolerances are exact equality and the referee
bound  max|kernel - fp64| <= c * max|torch fp32 - fp64| + one ulp  with c = HEAD_REFEREE_C.
"""
import functools
import types
import zlib
from collections import namedtuple

import torch

import env_exact_cases as ex
import kernel_checks as kc
from kernel_checks import (ALLOC_FACTORS, B_LANES64, B_LANES256, EPS32, HEAD_REFEREE_C, NAN, PREFILL, filled, grid_values, kernel_is,
                           out_ld, padding_untouched, referee, same_bits, soa)
from neural_inventory_control_amd import _lib, layout
from neural_inventory_control_amd.layout import EnvProblem, Table, ref_view, to_soa

NIC_SEG_MAX_TERMS = 4      # include/nic_rollout.h
K_ALLOC_BATCH = 8          # csrc/gnn_alloc_body.h: kAllocBatch
WIDE = HEAD_REFEREE_C["wide"]


def _seed(cid):
    return torch.Generator().manual_seed(zlib.crc32(cid.encode()))


def ceil4(n):
    return (n + 3) // 4 * 4


# ==== segment sums ===============================================================================================================
# path: "vec" (segment_sum*_kernel<4>: every row 16-byte aligned, ldb % 4 == 0) | "ld" (<1>: a last dimension that is no multiple of
# 4) | "offset-dst" / "offset-src" (<1>: a contiguous tensor carved out of a flat buffer one float past a 16-byte boundary).
# hist: the source is period 1 of a [R][3][n_src][ldb] history block (row stride 3 * n_src * ldb).  scale: None | "dyadic" | "sqrt5".
SEG_LENS = (3, 0, 1, 5, 4, 8, 9, 17)     # below, at and beyond the batch of four loads; 17 = the warehouse node's degree
N_SRC = 19
B_VEC = B_LANES256 + (1023, 1024, 1025, 1028)      # <4>: 256 lanes x 4 scenarios
SegCase = namedtuple("SegCase", "id family R B path hist accumulate scale")
TermsCase = namedtuple("TermsCase", "id family pattern R B path hist accumulate scale")   # pattern: "S" segment term, "P" plain term


def _seg_table():
    t, Rs = [], (1, 32, 33, 70)
    for i, B in enumerate(B_VEC):
        t.append(SegCase(f"vec-B{B}-R{Rs[i % 4]}", "grid", Rs[i % 4], B, "vec", i % 2 == 1, i % 3 == 0, (None, "dyadic")[i % 2]))
    for i, B in enumerate(B_LANES256):
        t.append(SegCase(f"ld-B{B}-R{Rs[(i + 1) % 4]}", "grid", Rs[(i + 1) % 4], B, "ld", i % 2 == 0, i % 2 == 1, ("dyadic", None)[i % 2]))
        path = ("offset-dst", "offset-src")[i % 2]
        t.append(SegCase(f"{path}-B{B}-R{Rs[(i + 2) % 4]}", "grid", Rs[(i + 2) % 4], B, path, i % 3 == 0, i % 2 == 0, "dyadic"))
    t.append(SegCase("random-vec", "random", 33, 600, "vec", True, True, "sqrt5"))
    t.append(SegCase("random-ld", "random", 70, 257, "ld", False, False, "sqrt5"))
    assert len({c.id for c in t}) == len(t)
    return t


def _terms_table():
    t, Rs = [], (1, 32, 33, 70)
    pats = ("S", "P", "SP", "PS", "SPS", "PSP", "SSPP", "PPSS", "SPSP", "PSPS")
    paths = ("vec", "ld", "vec", "offset-dst", "vec", "offset-src")
    i = 0
    for pat in pats:
        for acc in ((False, True) if len(pat) <= 2 else (len(pat) % 2 == 0,)):      # a first term of each kind with and without
            path = paths[i % len(paths)]
            B = (B_VEC if path == "vec" else B_LANES256)[i % (9 if path == "vec" else 5)]
            t.append(TermsCase(f"{pat}-{'acc' if acc else 'set'}-{path}-B{B}", "grid", pat, Rs[i % 4], B, path, i % 2 == 0, acc, "dyadic"))
            i += 1
    t.append(TermsCase("random-SPSP-vec", "random", "SPSP", 33, 600, "vec", True, False, "sqrt5"))
    t.append(TermsCase("random-PSS-ld", "random", "PSS", 70, 257, "ld", False, True, "sqrt5"))
    assert len({c.id for c in t}) == len(t)
    return t


SEG_CASES, TERMS_CASES = _seg_table(), _terms_table()


def seg_ldb(c):
    if c.path == "ld":
        return c.B + 1 if (c.B + 1) % 4 else c.B + 2
    return ceil4(c.B) + 4


def seg_expected_kernel(c):
    return ("segment_sum_terms_kernel" if isinstance(c, TermsCase) else "segment_sum_kernel") + ("<4>" if c.path == "vec" else "<1>")


def _segments(gen, lens, n_src):
    """offsets / items of one term: random items, one item twice in the first segment that has three, one item shared by two"""
    lists = [torch.randint(0, n_src, (n,), generator=gen).tolist() for n in lens]
    big = [l for l in lists if len(l) >= 3]
    big[0][1] = big[0][0]
    big[1][0] = big[0][0]
    offsets = [0]
    for l in lists:
        offsets.append(offsets[-1] + len(l))
    return lists, torch.tensor(offsets, dtype=torch.int32), torch.tensor([i for l in lists for i in l], dtype=torch.int32)


def _values(gen, family, shape):
    return grid_values(gen, shape, -3, 3) if family == "grid" else torch.randn(shape, generator=gen)


def _scales(gen, kind, n):
    if kind is None:
        return None
    if kind == "dyadic":
        return torch.tensor([0.25, 0.5, 1.0, 2.0])[torch.randint(0, 4, (n,), generator=gen)]
    return torch.full((n,), 1 / 5 ** 0.5)      # the 1 / sqrt(degree) of a node of degree 5, rounded to float32


@functools.lru_cache(maxsize=4)
def seg_problem(c):
    """CPU inputs ([R][.][ldb], every column filled: the 16-byte path sums the padding columns below (B + 3) / 4 * 4 too), and the
    float64 / float32 references of the live columns."""
    gen = _seed(c.id)
    ldb, n_dst = seg_ldb(c), len(SEG_LENS)
    pattern = c.pattern if isinstance(c, TermsCase) else "S"
    terms = []
    for j, kind in enumerate(pattern):
        lens = SEG_LENS[j:] + SEG_LENS[:j]
        if kind == "S":
            lists, offsets, items = _segments(gen, lens, N_SRC)
            src = _values(gen, c.family, (c.R, 3 if c.hist else 1, N_SRC, ldb))
        else:
            lists, offsets, items = [[n] for n in range(n_dst)], None, None
            src = _values(gen, c.family, (c.R, 3 if c.hist else 1, n_dst, ldb))
        terms.append(dict(kind=kind, lists=lists, offsets=offsets, items=items, src=src, scale=_scales(gen, c.scale if (kind == "S" or c.family == "grid") else None, n_dst)))
    prefill = _values(gen, c.family, (c.R, n_dst, ldb)) if c.accumulate else torch.full((c.R, n_dst, ldb), NAN)
    p = dict(case=c, ldb=ldb, terms=terms, prefill=prefill)

    def expression(dtype):
        acc = prefill[:, :, :c.B].to(dtype) if c.accumulate else torch.zeros(c.R, n_dst, c.B, dtype=dtype)
        for t in terms:
            s = t["src"][:, 1 if c.hist else 0, :, :c.B].to(dtype)
            summed = torch.stack([s[:, l].sum(dim=1) if l else torch.zeros(c.R, c.B, dtype=dtype) for l in t["lists"]], dim=1)
            if t["scale"] is not None:
                summed = summed * t["scale"].to(dtype)[None, :, None]
            acc = acc + summed
        return acc
    p["ref64"], p["ref32"] = expression(torch.float64), expression(torch.float32)
    if c.family == "grid":      # exact inputs and dyadic scales: the float64 result IS a float32
        assert torch.equal(p["ref64"].float().double(), p["ref64"]), (c.id, "the grid family's result is not a float32")
    return p


def _carve(shape, values, dev, misalign):
    """a contiguous device tensor holding `values`, 16-byte aligned or (misalign) one float past a 16-byte boundary"""
    n = values.numel()
    flat = torch.empty(n + 8, dtype=torch.float32, device=dev)
    want = 4 if misalign else 0
    off = next(o for o in range(4) if (flat.data_ptr() + 4 * o) % 16 == want)
    t = flat[off:off + n].view(shape)
    t.copy_(values.to(dev))
    assert t.data_ptr() % 16 == want and t.is_contiguous()
    return t


def _seg_buffers(p, dev):
    c = p["case"]
    dst = _carve(p["prefill"].shape, p["prefill"], dev, c.path == "offset-dst")
    srcs = []
    for j, t in enumerate(p["terms"]):
        full = _carve(t["src"].shape, t["src"], dev, c.path == "offset-src" and j == 0)
        srcs.append((full, full[:, 1 if c.hist else 0]))      # the view the launch gets: rows full.stride(0) apart
    i32 = lambda x: None if x is None else x.to(dev)  # noqa: E731
    terms = [(v, i32(t["offsets"]), i32(t["items"]), i32(t["scale"])) for (_, v), t in zip(srcs, p["terms"])]
    return dst, srcs, terms


def _seg_verify(be, c, p, dst, before, srcs, kernel):
    kernel_is(be, kernel, c.id)
    # the 16-byte path owns the columns below (B + 3) / 4 * 4 (its launcher says so); everything behind is nobody's
    padding_untouched(dst, before, ceil4(c.B) if c.path == "vec" else c.B, (c.id, "dst"))
    for (full, _), t in zip(srcs, p["terms"]):
        assert torch.equal(full.cpu(), t["src"]), (c.id, "a source was written")
    got = dst[:, :, :c.B].cpu()
    if c.family == "grid":
        assert torch.equal(got, p["ref64"].float()), (c.id, "not bit-equal to float64", int((got != p["ref64"].float()).sum()))
    else:
        referee(be, kernel.split("<")[0], "dst", got, p["ref32"], p["ref64"], WIDE, c.id)


def check_segment_sum(be, c):
    p = seg_problem(c)
    dst, srcs, terms = _seg_buffers(p, be.device)
    before = dst.clone()
    src, offsets, items, scale = terms[0]
    be.segment_sum(dst, src, offsets, items, scale, c.R, len(SEG_LENS), c.B, p["ldb"], c.accumulate)
    be.sync()
    _seg_verify(be, c, p, dst, before, srcs, seg_expected_kernel(c))


def check_segment_sum_terms(be, c):
    p = seg_problem(c)
    dev, n_dst = be.device, len(SEG_LENS)
    dst, srcs, terms = _seg_buffers(p, dev)
    before = dst.clone()
    be.segment_sum_terms(dst, terms, c.R, n_dst, c.B, p["ldb"], c.accumulate)
    be.sync()
    _seg_verify(be, c, p, dst, before, srcs, seg_expected_kernel(c))
    # ... and the values of the chain of nic_segment_sum(accumulate) launches it replaces (a plain addend = a segment of its own
    # row), bit for bit: with a non-dyadic scale the order of the terms shows in the last bit
    chain = before.clone()
    ident_o, ident_i = torch.arange(n_dst + 1, dtype=torch.int32, device=dev), torch.arange(n_dst, dtype=torch.int32, device=dev)
    for j, (src, offsets, items, scale) in enumerate(terms):
        o, i = (offsets, items) if offsets is not None else (ident_o, ident_i)
        be.segment_sum(chain, src, o, i, scale, c.R, n_dst, c.B, p["ldb"], c.accumulate or j > 0)
    be.sync()
    assert torch.equal(dst[:, :, :c.B], chain[:, :, :c.B]), (c.id, "differs from the chain of segment-sum launches")


# ==== proportional allocation: one warehouse and groups ==========================================================================
# A group = (member rows of `out`, self-loop row or -1, supplier row, order row of each member, order row of the supplier's own).
AllocCase = namedtuple("AllocCase", "id family S e_self cap n_edges B")
GroupsCase = namedtuple("GroupsCase", "id family counts selfs Ww zero_count cap B")


def _alloc_table():
    t, i = [], 0
    for S in (1, 7, 8, 9, 16, 17, 64, 70):
        for e_self in (False, True):
            for cap in (False, True):
                # S stores, the self loop, the supplier edge and demand edges up to the next n_edges % 8 in {0, 1}
                n_edges = S + 3
                while n_edges % 8 != i % 2:
                    n_edges += 1
                t.append(AllocCase(f"grid-S{S}-self{int(e_self)}-cap{int(cap)}", "grid", S, e_self, cap, n_edges, B_LANES64[i % 5]))
                t.append(AllocCase(f"random-S{S}-self{int(e_self)}-cap{int(cap)}", "random", S, e_self, cap, n_edges, B_LANES64[2 + i % 3]))
                i += 1
    assert len({c.id for c in t}) == len(t)
    return t


def _groups_table():
    t = []
    shapes = (("G1-9", (9,), (True,), 1, 0), ("G1-self-only", (0,), (True,), 3, 2),
              ("G3", (8, 0, 1), (False, False, True), 3, 2), ("G5", (9, 0, 8, 0, 1), (True, True, False, False, True), 1, 3),
              ("G3-w1", (1, 9, 8), (True, False, True), 1, 0))
    for i, (name, counts, selfs, Ww, zc) in enumerate(shapes):
        for cap in (False, True):
            t.append(GroupsCase(f"grid-{name}-cap{int(cap)}", "grid", counts, selfs, Ww, zc, cap, B_LANES64[(2 * i + cap) % 5]))
        t.append(GroupsCase(f"random-{name}", "random", counts, selfs, Ww, zc, i % 2 == 0, B_LANES64[2 + i % 3]))
    assert len({c.id for c in t}) == len(t)
    return t


ALLOC_CASES, GROUPS_CASES = _alloc_table(), _groups_table()


def alloc_layout(c):
    """-> (n_edges, groups [(members, e_self, e_sup, member order rows, supplier order row)], n order rows, zero_first, order_row)"""
    if isinstance(c, AllocCase):
        S = c.S
        e_self = S + 1 if c.e_self else -1
        return c.n_edges, [(list(range(S)), e_self, c.n_edges - 1, list(range(S)), S)], S + 1, None, None
    G, n_int = len(c.counts), sum(c.counts)
    # rows of `out`: the members of each group (contiguous), the supplier edges, the demand edges, the self loops
    e_dem = n_int + G
    n_edges = e_dem + c.zero_count + sum(c.selfs)
    perm = torch.randperm(n_int + G, generator=_seed("perm" + c.id.split("-", 1)[1])).tolist()     # a permuted edge -> order row map
    order_row = torch.full((n_edges,), -1, dtype=torch.int32)
    order_row[:n_int + G] = torch.tensor(perm, dtype=torch.int32)
    groups, first, e_next_self = [], 0, e_dem + c.zero_count
    for g, (cnt, has_self) in enumerate(zip(c.counts, c.selfs)):
        members = list(range(first, first + cnt))
        e_self = -1
        if has_self:
            e_self, e_next_self = e_next_self, e_next_self + 1
        groups.append((members, e_self, n_int + g, [perm[e] for e in members], perm[n_int + g]))
        first += cnt
    return n_edges, groups, n_int + G, e_dem, order_row


def _alloc_expression(p, dtype):
    """apply_proportional_allocation (neural_networks.py:111-138) per supplying node in aten ops + autograd, in `dtype`"""
    c = p["case"]
    o, h = p["out"].to(dtype).requires_grad_(True), p["on_hand"].to(dtype).requires_grad_(True)
    g_orders = p["g_orders"].to(dtype)
    G, B = len(p["groups"]), o.shape[1]
    rows = [None] * p["n_rows"]
    sums, ratio, scale = (torch.full((G, B), NAN, dtype=dtype) for _ in range(3))
    den = torch.zeros(o.shape, dtype=dtype)       # |common| + |g * scale| per element of d_out (0: no cancellation behind it)
    for g, (members, e_self, e_sup, mrows, srow) in enumerate(p["groups"]):
        rows[srow] = o[e_sup]
        idx = members + ([e_self] if e_self >= 0 else [])
        if not idx:
            continue
        sm = o[idx].sum(dim=0)
        r = h[g] / (sm + EPS32)
        sc = torch.clamp(r, max=1.0) if c.cap else r
        sums[g], ratio[g], scale[g] = sm.detach(), r.detach(), sc.detach()
        for e, row in zip(members, mrows):
            rows[row] = o[e] * sc
        with torch.no_grad():
            dot = sum((g_orders[row] * o[e] for e, row in zip(members, mrows)), torch.zeros(B, dtype=dtype))
            passes = (r <= 1).to(dtype) if c.cap else torch.ones(B, dtype=dtype)
            common = (dot * passes * h[g] / (sm + EPS32) ** 2).abs()
            for e, row in zip(members, mrows):
                den[e] = common + (g_orders[row] * sc).abs()
            if e_self >= 0:
                den[e_self] = common
    orders = torch.stack(rows)
    (orders * g_orders).sum().backward()
    g_oh = h.grad if h.grad is not None else torch.zeros_like(h)
    return dict(orders=orders.detach(), sums=sums, ratio=ratio, scale=scale, d_out=o.grad, g_on_hand=g_oh, den=den)


def _alloc_inputs(c, gen, n_edges, groups, n_rows, B):
    """out [n_edges][B], on_hand [G][B], g_orders [n_rows][B] of either family"""
    b = torch.arange(B)
    zero_scn = b % 7 == 6
    if c.family == "grid":
        out = grid_values(gen, (n_edges, B), 0, 3)
        out[torch.rand(n_edges, B, generator=gen) < 0.25] = 0.0
        g_orders = grid_values(gen, (n_rows, B), -2, 2, 4)
        factors = torch.tensor(ALLOC_FACTORS, dtype=torch.float64)[b % 6]
    else:
        out = torch.rand(n_edges, B, generator=gen) * 3 + 0.01
        g_orders = torch.randn(n_rows, B, generator=gen)
        factors = None
    on_hand = torch.zeros(len(groups), B, dtype=torch.float64)
    for g, (members, e_self, _, _, _) in enumerate(groups):
        idx = members + ([e_self] if e_self >= 0 else [])
        if not idx:
            on_hand[g] = 1.0      # (never read: a group that supplies nobody)
            continue
        if c.family == "grid":
            out[torch.tensor(idx)[:, None], b[zero_scn][None, :]] = 0.0        # every 7th scenario: nobody asks, stock 2
            on_hand[g] = torch.where(zero_scn, 2.0, out[idx].double().sum(dim=0) * factors)
        else:
            on_hand[g] = out[idx].double().sum(dim=0) * kc.stock_factors(gen, B)
    return out, on_hand.float(), g_orders, factors, zero_scn


@functools.lru_cache(maxsize=None)
def alloc_problem(c):
    n_edges, groups, n_rows, zero_first, order_row = alloc_layout(c)
    out, on_hand, g_orders, factors, zero_scn = _alloc_inputs(c, _seed(c.id), n_edges, groups, n_rows, c.B)
    p = dict(case=c, n_edges=n_edges, groups=groups, n_rows=n_rows, zero_first=zero_first, order_row=order_row, out=out, on_hand=on_hand,
             g_orders=g_orders)
    p["ref64"], p["ref32"] = _alloc_expression(p, torch.float64), _alloc_expression(p, torch.float32)
    if c.family == "grid":
        assert_grid_family(p, factors, zero_scn)
    return p


def assert_grid_family(p, factors, zero_scn):
    """the grid family's conditions on the reference alone (kernel_checks.assert_grid_allocation) + the orders on the 1/32 grid"""
    c, r = p["case"], p["ref64"]
    assert torch.equal(p["on_hand"].double(), p["on_hand"].double().float().double())
    for g, (members, e_self, _, _, _) in enumerate(p["groups"]):
        idx = members + ([e_self] if e_self >= 0 else [])
        if idx:
            kc.assert_grid_allocation(r["sums"][g], [p["out"][e] for e in idx], r["ratio"][g], factors, zero_scn, (c.id, g))
    o32 = r["orders"].float().double()
    assert torch.equal(o32 * 32, (o32 * 32).round()), (c.id, "orders off the 1/32 grid")


def alloc_planted(c):
    p = alloc_problem(c)
    r = p["ref64"]
    live = ~torch.isnan(r["ratio"])
    return {"tie": bool((r["ratio"].float()[live] == 1).any()), "all_zero_with_stock": bool(((r["sums"] == 0) & (r["ratio"] > 1))[live].any()),
            "self_loop_without_members": any(not m and s >= 0 for m, s, _, _, _ in p["groups"]),
            "neither_self_loop_nor_members": any(not m and s < 0 for m, s, _, _, _ in p["groups"])}


def _check_alloc_forward(be, c, p, got, kernel):
    """got: {orders [n_rows][B], sums / ratio / scale [G][B]} (CPU)"""
    r64, r32 = p["ref64"], p["ref32"]
    live = ~torch.isnan(r64["ratio"][:, 0])
    for g, (_, _, _, _, srow) in enumerate(p["groups"]):
        assert torch.equal(got["orders"][srow], r64["orders"][srow].float()), (c.id, g, "the supplier's own order does not pass through")
    for name in ("orders", "sums", "ratio", "scale"):
        rows = slice(None) if name == "orders" else live
        if c.family == "grid":
            assert torch.equal(got[name][rows], r64[name][rows].float()), (c.id, name, "not bit-equal to float64")
        else:
            referee(be, kernel, name, got[name][rows], r32[name][rows], r64[name][rows], WIDE, c.id)


def _check_alloc_backward(be, c, p, d_out, inc, inc32, kernel, nobody):
    """d_out [n_edges][B] (pre-filled with NaN), inc = g_on_hand - PREFILL [G][B]; nobody: rows of d_out no lane owns (still NaN)"""
    r64, r32 = p["ref64"], p["ref32"]
    if nobody:
        assert bool(torch.isnan(d_out[nobody]).all()), (c.id, "a row of d_out nobody owns was written")
    owned = [e for e in range(p["n_edges"]) if e not in nobody]
    got, want, want32, den = d_out[owned], r64["d_out"][owned], r32["d_out"][owned], r64["den"][owned]
    assert not bool(torch.isnan(got).any()), (c.id, "a row of d_out was left unwritten")
    flat = den == 0      # nothing cancels behind these: structural zeros, the supplier's pass-through row
    assert torch.equal(got[flat].double(), want[flat]), (c.id, "d_out: a structurally zero / pass-through element is not exact")
    if bool((~flat).any()):      # relative to |common| + |g * scale| of the float64 reference
        rel = lambda x: (x.double() - want)[~flat] / den[~flat]  # noqa: E731
        _referee_relative(be, kernel, "d_out", rel(got), rel(want32), c.id)
    live = ~torch.isnan(r64["ratio"][:, 0])
    referee(be, kernel, "g_on_hand", inc[live], inc32[live], r64["g_on_hand"][live], WIDE, c.id)


def _referee_relative(be, kernel, tensor, rel_k, rel_t, what):
    """the referee bound on errors already divided by the element's magnitude (one ulp of 1 as the absolute term)"""
    err_k, err_t, ulp = float(rel_k.detach().abs().max()), float(rel_t.detach().abs().max()), kc._ulp(1.0)
    ratio = err_k / err_t if err_t > 0 else (0.0 if err_k == 0 else float("inf"))
    key = (type(be).__name__, kernel, tensor)
    if ratio != float("inf"):
        kc.REFEREE_FIGURES[key] = max(kc.REFEREE_FIGURES.get(key, 0.0), ratio)
    print(f"referee {what} {key[0]} {kernel} {tensor} (relative): kernel {err_k:.3e} torch32 {err_t:.3e} ratio {ratio:.2f} c {WIDE}")
    assert err_k <= WIDE * err_t + ulp, (what, kernel, tensor, "kernel", err_k, "torch32", err_t, "ulp", ulp, "c", WIDE)


def check_alloc(be, c):
    """nic_gnn_alloc_fwd / _bwd on one case of ALLOC_CASES"""
    p = alloc_problem(c)
    dev, B, S = be.device, c.B, c.S
    ld = out_ld(B)
    (members, e_self, e_sup, _, _), = p["groups"]
    out, on_hand = soa(p["out"], ld, dev), soa(p["on_hand"][0], ld, dev)
    orders, sums, ratio, scale = filled((S + 1, ld), NAN, dev), filled((ld,), NAN, dev), filled((ld,), NAN, dev), filled((ld,), NAN, dev)
    outs = (orders, sums, ratio, scale)
    before = [x.clone() for x in outs]
    be.alloc_fwd(out, on_hand, orders, sums, ratio, scale, S, e_self, e_sup, c.cap, B, ld)
    be.sync()
    kernel_is(be, "gnn_alloc_fwd_kernel", c.id)
    for x, b4, name in zip(outs, before, ("orders", "sums", "ratio", "scale")):
        padding_untouched(x, b4, B, (c.id, name))
    got = dict(orders=orders[:, :B].cpu(), sums=sums[None, :B].cpu(), ratio=ratio[None, :B].cpu(), scale=scale[None, :B].cpu())
    _check_alloc_forward(be, c, p, got, "gnn_alloc_fwd")
    d_out, g_on = filled((p["n_edges"], ld), NAN, dev), filled((ld,), PREFILL, dev)
    before = [d_out.clone(), g_on.clone()]
    be.alloc_bwd(out, on_hand, soa(p["g_orders"], ld, dev), sums, ratio, scale, d_out, g_on, S, p["n_edges"], e_self, e_sup, c.cap, B, ld)
    be.sync()
    kernel_is(be, "gnn_alloc_bwd_kernel", c.id)
    padding_untouched(d_out, before[0], B, (c.id, "d_out"))
    padding_untouched(g_on, before[1], B, (c.id, "g_on_hand"))
    inc = g_on[None, :B].cpu().double() - PREFILL
    inc32 = (p["ref32"]["g_on_hand"] + torch.tensor(PREFILL)).double() - PREFILL
    _check_alloc_backward(be, c, p, d_out[:, :B].cpu(), inc, inc32, "gnn_alloc_bwd", [])


def check_alloc_groups(be, c):
    """nic_gnn_alloc_groups_fwd / _bwd on one case of GROUPS_CASES"""
    p = alloc_problem(c)
    dev, B, G, Ww = be.device, c.B, len(c.counts), c.Ww
    ld = out_ld(B)
    out = soa(p["out"], ld, dev)
    on_hand = filled((G, Ww, ld), 0.0, dev)
    on_hand[:, 0, :B] = p["on_hand"].to(dev)
    groups = torch.tensor([[m[0] if m else 0, len(m), e_self, e_sup] for m, e_self, e_sup, _, _ in p["groups"]], dtype=torch.int32, device=dev)
    order_row = p["order_row"].to(dev)
    orders = filled((p["n_rows"], ld), NAN, dev)
    sums, ratio, scale = (filled((G, ld), NAN, dev) for _ in range(3))
    outs = (orders, sums, ratio, scale)
    before = [x.clone() for x in outs]
    be.groups_fwd(out, on_hand, orders, sums, ratio, scale, groups, order_row, c.cap, B, ld)
    be.sync()
    kernel_is(be, "gnn_alloc_groups_fwd_kernel", c.id)
    for x, b4, name in zip(outs, before, ("orders", "sums", "ratio", "scale")):
        padding_untouched(x, b4, B, (c.id, name))
    idle = [g for g, (m, e_self, _, _, _) in enumerate(p["groups"]) if not m and e_self < 0]
    for x, b4, name in zip(outs[1:], before[1:], ("sums", "ratio", "scale")):      # a group that supplies nobody: its own order only
        assert same_bits(x[idle], b4[idle]), (c.id, name, "written for a group without members and self loop")
    got = dict(orders=orders[:, :B].cpu(), sums=sums[:, :B].cpu(), ratio=ratio[:, :B].cpu(), scale=scale[:, :B].cpu())
    _check_alloc_forward(be, c, p, got, "gnn_alloc_groups_fwd")
    d_out, g_on = filled((p["n_edges"], ld), NAN, dev), filled((G, Ww, ld), PREFILL, dev)
    before = [d_out.clone(), g_on.clone()]
    be.groups_bwd(out, on_hand, soa(p["g_orders"], ld, dev), sums, ratio, scale, d_out, g_on, groups, order_row, p["zero_first"], c.zero_count,
                  c.cap, B, ld)
    be.sync()
    kernel_is(be, "gnn_alloc_groups_bwd_kernel", c.id)
    padding_untouched(d_out, before[0], B, (c.id, "d_out"))
    padding_untouched(g_on, before[1], B, (c.id, "g_on_hand"))
    assert same_bits(g_on[:, 1:], before[1][:, 1:]), (c.id, "g_on_hand: a pipeline slot behind the on-hand one was written")
    assert same_bits(g_on[idle], before[1][idle]), (c.id, "g_on_hand of a group that supplies nobody was written")
    inc = g_on[:, 0, :B].cpu().double() - PREFILL
    inc32 = (p["ref32"]["g_on_hand"] + torch.tensor(PREFILL)).double() - PREFILL
    _check_alloc_backward(be, c, p, d_out[:, :B].cpu(), inc, inc32, "gnn_alloc_groups_bwd", [])


# ==== the fused allocation + env step ============================================================================================
AllocEnvCase = namedtuple("AllocEnvCase", "id seed S B Ws Ww lost profit per_scenario e_self cap")


def _alloc_env_table():
    rows = (  # S, B, (Ws, Ww), lost, profit, per-scenario tables, self loop, cap
        (1, 1, (2, 2), True, False, False, False, True), (3, 63, (4, 4), True, False, True, True, True),
        (4, 64, (5, 3), False, False, False, True, False), (5, 65, (3, 8), True, True, True, False, True),
        (16, 130, (9, 2), False, True, False, True, True), (17, 1, (16, 16), True, False, True, True, False),
        (33, 63, (2, 2), False, True, True, False, False), (1, 64, (4, 4), False, False, True, True, True),
        (3, 65, (5, 3), True, True, False, False, False), (4, 130, (3, 8), False, True, True, True, True),
        (5, 1, (9, 2), True, False, False, True, True), (16, 63, (16, 16), False, False, True, False, True),
        (17, 64, (2, 2), True, True, False, True, False), (33, 65, (4, 4), True, False, False, True, True),
        (1, 130, (5, 3), True, False, True, False, False), (3, 64, (3, 8), False, False, False, True, True),
        (4, 65, (9, 2), True, True, True, False, True), (5, 130, (16, 16), False, True, False, True, False),
        (16, 65, (4, 4), True, False, True, True, True), (17, 130, (3, 8), False, True, True, False, True),
        (33, 130, (9, 2), True, False, False, True, True))
    t = [AllocEnvCase(f"S{S}-B{B}-slots{a}-{b}-lost{int(lo)}-profit{int(pr)}-{'scn' if ps else 'uni'}-self{int(se)}-cap{int(cap)}",
                      900 + i, S, B, a, b, lo, pr, ps, se, cap) for i, (S, B, (a, b), lo, pr, ps, se, cap) in enumerate(rows)]
    assert len({c.id for c in t}) == len(t)
    return t


ALLOC_ENV_CASES = _alloc_env_table()


def alloc_env_variant(c):
    m = max(c.Ws, c.Ww)
    return 4 if m <= 4 else (8 if m <= 8 else _lib.NIC_MAX_SLOTS)


@functools.lru_cache(maxsize=None)
def alloc_env_problem(c):
    """A period of env_exact_cases.make_case (one warehouse, no echelons) whose orders are the grid family's allocation: desired
    quantities on the 1/8 grid, the warehouse's on-hand overwritten with sum * f.  The orders then sit on the 1/32 grid, and the
    period after them is exact: checked here on the reference alone (the oracle in float32 == the oracle in float64)."""
    k = ex.make_case(c.seed, c.B, c.S, 1, 0, c.Ws, c.Ww, 0, c.lost, c.profit, True, c.per_scenario)
    S, B = c.S, c.B
    n_edges = S + 5      # stores, the supplier edge, the self loop's row (used or not), three demand edges
    e_self, e_sup = (S + 1 if c.e_self else -1), S
    groups = [(list(range(S)), e_self, e_sup, list(range(S)), S)]
    ac = types.SimpleNamespace(id=c.id, family="grid", cap=c.cap)
    out, on_hand, g_orders, factors, zero_scn = _alloc_inputs(ac, _seed(c.id), n_edges, groups, S + 1, B)
    k["state"]["warehouse_inventories"][:, 0, 0] = on_hand[0]      # (the same tensor as data["initial_warehouse_inventories"])
    p = dict(case=ac, env_case=c, n_edges=n_edges, groups=groups, n_rows=S + 1, out=out, on_hand=on_hand, g_orders=g_orders, k=k,
             e_self=e_self, e_sup=e_sup)
    p["ref64"], p["ref32"] = _alloc_expression(p, torch.float64), _alloc_expression(p, torch.float32)
    assert_grid_family(p, factors, zero_scn)
    o32 = p["ref64"]["orders"].float()
    k["act"] = {"stores": o32[:S].t().contiguous()[:, :, None], "warehouses": o32[S][:, None, None].contiguous()}
    k["case"] = types.SimpleNamespace(Wn=1)
    r32, r64 = ex.oracle_period(k, torch.float32), ex.oracle_period(k, torch.float64)
    for n in r32:
        assert torch.equal(r32[n].double(), r64[n]), (c.id, n, "the oracle is not exact on the reference orders")
    p["oracle"] = r32
    return p


def check_alloc_env(be, c):
    """nic_gnn_alloc_env_fwd / _bwd on one case of ALLOC_ENV_CASES: (a) bit-identical to the separate launches, (b) the period after the
    allocation equal to the oracle on the reference orders"""
    p = alloc_env_problem(c)
    k, dev, S, B = p["k"], be.device, c.S, c.B
    prob = EnvProblem(k["problem"], k["data"], dev)
    ld = prob.ldb
    s, w = to_soa(k["state"]["store_inventories"].to(dev), ld), to_soa(k["state"]["warehouse_inventories"].to(dev), ld)
    dem_t = k["data"]["demands"].to(dev)
    dem = kc._demand_table(dem_t, 0)
    out = soa(p["out"], ld, dev)
    e_self, e_sup, n_edges = p["e_self"], p["e_sup"], p["n_edges"]
    variant = alloc_env_variant(c)

    def forward(fused):
        o = dict(orders=filled((S + 1, ld), NAN, dev), sums=filled((ld,), NAN, dev), ratio=filled((ld,), NAN, dev),
                 scale=filled((ld,), NAN, dev), store=filled(tuple(s.shape), NAN, dev), wh=filled(tuple(w.shape), NAN, dev),
                 reward=filled((ld,), NAN, dev))
        before = {n: x.clone() for n, x in o.items()}
        if fused:
            be.alloc_env_fwd(prob, s, w, dem, out, o["orders"], o["sums"], o["ratio"], o["scale"], e_self, e_sup, c.cap, o["store"], o["wh"],
                             o["reward"])
            be.sync()
            kernel_is(be, f"gnn_alloc_env_fwd_kernel<{variant}>", c.id)
        else:
            be.alloc_fwd(out, w[0, 0], o["orders"], o["sums"], o["ratio"], o["scale"], S, e_self, e_sup, c.cap, B, ld)
            be.env_fwd(prob, s, w, dem, o["orders"], o["store"], o["wh"], o["reward"])
            be.sync()
        for n, x in o.items():
            padding_untouched(x, before[n], B, (c.id, "fused" if fused else "separate", n))
        return o
    fu, se = forward(True), forward(False)
    for n in fu:
        assert torch.equal(fu[n][..., :B], se[n][..., :B]), (c.id, "forward", n, "fused differs from the two launches")
    got = dict(orders=fu["orders"][:, :B].cpu(), sums=fu["sums"][None, :B].cpu(), ratio=fu["ratio"][None, :B].cpu(),
               scale=fu["scale"][None, :B].cpu())
    _check_alloc_forward(be, p["case"], p, got, "gnn_alloc_env_fwd")
    want = p["oracle"]
    assert torch.equal(ref_view(fu["store"], B).cpu(), want["next_store_inventories"]), (c.id, "next store state != oracle")
    assert torch.equal(ref_view(fu["wh"], B).cpu(), want["next_warehouse_inventories"]), (c.id, "next warehouse state != oracle")
    assert torch.equal(fu["reward"][:B].cpu(), want["reward"]), (c.id, "reward != oracle")

    gso, gwo = to_soa(k["g_out"]["store_inventories"].to(dev), ld), to_soa(k["g_out"]["warehouse_inventories"].to(dev), ld)
    grs = torch.zeros(ld, device=dev)
    grs[:B] = k["g_reward"].to(dev)
    gr = layout.Table(grs, 0, 1)

    def backward(fused):
        o = dict(g_store=filled(tuple(s.shape), NAN, dev), g_wh=filled(tuple(w.shape), NAN, dev), g_orders=filled((S + 1, ld), NAN, dev),
                 d_out=filled((n_edges, ld), NAN, dev))
        before = {n: x.clone() for n, x in o.items()}
        if fused:
            be.alloc_env_bwd(prob, s, w, dem, out, fu["orders"], fu["sums"], fu["ratio"], fu["scale"], e_self, e_sup, c.cap, gso, gwo, gr,
                             o["g_store"], o["g_wh"], o["g_orders"], o["d_out"])
            be.sync()
            kernel_is(be, f"gnn_alloc_env_bwd_kernel<{variant}>", c.id)
        else:
            be.env_bwd(prob, s, w, dem, fu["orders"], gso, gwo, gr, o["g_store"], o["g_wh"], o["g_orders"])
            be.alloc_bwd(out, w[0, 0], o["g_orders"], fu["sums"], fu["ratio"], fu["scale"], o["d_out"], o["g_wh"][0, 0], S, n_edges, e_self,
                         e_sup, c.cap, B, ld)
            be.sync()
        for n, x in o.items():
            padding_untouched(x, before[n], B, (c.id, "fused" if fused else "separate", n))
        return o
    fb, sb = backward(True), backward(False)
    for n in fb:
        assert same_bits(fb[n][..., :B], sb[n][..., :B]), (c.id, "backward", n, "fused differs from the two launches")
    assert not bool(torch.isnan(fb["d_out"][:, :B]).any()), (c.id, "a row of d_out was left unwritten")
    # the order gradients of the env adjoint are the oracle's (exact period), and the rows of d_out nothing feeds are exact zeros
    assert torch.equal(ref_view(fb["g_orders"][:S], B).cpu(), want["g_act_stores"][:, :, 0]), (c.id, "g_orders != oracle")
    zero_rows = [e for e in range(n_edges) if e >= S and e not in (e_self, e_sup)]
    assert bool((fb["d_out"][zero_rows][:, :B] == 0).all()), (c.id, "d_out rows that feed nothing are not exact zeros")
    assert torch.equal(fb["d_out"][e_sup, :B], fb["g_orders"][S, :B]), (c.id, "the supplier edge's gradient does not pass through")


# ==== nic_round_orders ============================================================================================================
RoundCase = namedtuple("RoundCase", "id rows B")
ROUND_CASES = [RoundCase(f"rows{r}-B{B}", r, B) for r, B in ((1, 1), (64, 255), (65, 256), (130, 257), (1, 600), (65, 1), (130, 600), (64, 257))]
ROUND_VALUES = (0.5, 1.5, 2.5, 3.5, -0.5, -1.5, -2.5, -0.25, -0.49, 0.49, 2.0 ** 23, 2.0 ** 23 + 1, 2.0 ** 24, -(2.0 ** 23) - 1, 1e9,
                8388607.5, 4194303.5, 4194304.5, 0.0, -0.0)


@functools.lru_cache(maxsize=None)
def round_problem(c):
    gen = _seed(c.id)
    x = torch.rand(c.rows, c.B, generator=gen) * 40 - 20
    half = torch.rand(c.rows, c.B, generator=gen) < 0.3
    x[half] = torch.randint(-9, 9, (int(half.sum()),), generator=gen).float() + 0.5       # k + 0.5, k even and odd, both signs
    flat = x.view(-1)
    sp = torch.tensor(ROUND_VALUES)
    n = min(flat.numel(), len(sp))
    shift = zlib.crc32(c.id.encode()) % len(sp)
    flat[:n] = sp.roll(shift)[:n]
    return x


def check_round_orders(be, c):
    x = round_problem(c)
    ld = out_ld(c.B)
    buf = soa(x, ld, be.device, fill=0.5)      # a touched padding column shows: 0.5 rounds to 0
    before = buf.clone()
    be.round_orders(buf, c.rows, c.B, ld)
    be.sync()
    kernel_is(be, "round_orders_kernel", c.id)
    padding_untouched(buf, before, c.B, (c.id, "orders"))
    assert torch.equal(buf[:, :c.B].cpu(), torch.round(x)), (c.id, "differs from torch.round (half to even)")


# ==== what the tables must reach ==================================================================================================

def expected_kernel_names():
    """every kernel name some case of the tables (here and in kernel_checks.py) expects from nic_last_kernel()"""
    names = {seg_expected_kernel(c) for c in SEG_CASES + TERMS_CASES}
    names |= {"gnn_alloc_fwd_kernel", "gnn_alloc_bwd_kernel"} if ALLOC_CASES else set()
    names |= {"gnn_alloc_groups_fwd_kernel", "gnn_alloc_groups_bwd_kernel"} if GROUPS_CASES else set()
    for c in ALLOC_ENV_CASES:
        names |= {f"gnn_alloc_env_fwd_kernel<{alloc_env_variant(c)}>", f"gnn_alloc_env_bwd_kernel<{alloc_env_variant(c)}>"}
    for cases, stem in ((kc.DATA_DRIVEN_CASES, "head_data_driven"), (kc.SERIAL_CASES, "head_serial"), (kc.SOFTPLUS_CASES, "head_softplus")):
        names |= {f"{stem}_fwd_kernel", f"{stem}_bwd_kernel"} if cases else set()
    names |= {"round_orders_kernel"} if ROUND_CASES else set()
    return names


ALL_LAUNCHER_CELLS = ({f"segment_sum_kernel<{v}>" for v in (1, 4)} | {f"segment_sum_terms_kernel<{v}>" for v in (1, 4)}
                      | {f"gnn_alloc{g}_{d}_kernel" for g in ("", "_groups") for d in ("fwd", "bwd")}
                      | {f"gnn_alloc_env_{d}_kernel<{m}>" for d in ("fwd", "bwd") for m in (4, 8, 16)}
                      | {f"head_{h}_{d}_kernel" for h in ("data_driven", "serial", "softplus") for d in ("fwd", "bwd")}
                      | {"round_orders_kernel"})


# ==== backend 1: the HIP kernels ==================================================================================================

class HipGlue(kc.HipBackend):
    """the product library: the C ABI where a case needs n_scenarios < ldb (ops.segment_sum passes ldb for both), ops elsewhere"""

    def __init__(self):
        super().__init__()
        from neural_inventory_control_amd import ops
        self.ops = ops

    def segment_sum(self, dst, src, offsets, items, scale, R, n_dst, B, ldb, accumulate):
        P = kc.P
        _lib.check(self.l.nic_segment_sum(P(dst), dst.stride(0), P(src), src.stride(0), P(offsets), P(items), P(scale), R, n_dst, B, ldb,
                                          int(accumulate), self._s()))

    def segment_sum_terms(self, dst, terms, R, n_dst, B, ldb, accumulate):
        P = kc.P
        arr = (_lib.NicSegTerm * len(terms))()
        for j, (src, offsets, items, scale) in enumerate(terms):
            arr[j].src, arr[j].src_row_stride = P(src), src.stride(0)
            arr[j].offsets, arr[j].items, arr[j].scale = P(offsets), P(items), P(scale)
        _lib.check(self.l.nic_segment_sum_terms(P(dst), dst.stride(0), arr, len(terms), R, n_dst, B, ldb, int(accumulate), self._s()))

    def alloc_fwd(self, out, on_hand, orders, sums, ratio, scale, S, e_self, e_sup, cap, B, ldb):
        P = kc.P
        _lib.check(self.l.nic_gnn_alloc_fwd(P(out), P(on_hand), P(orders), P(sums), P(ratio), P(scale), S, e_self, e_sup, int(cap), B, ldb,
                                            self._s()))

    def alloc_bwd(self, out, on_hand, g_orders, sums, ratio, scale, d_out, g_on_hand, S, n_edges, e_self, e_sup, cap, B, ldb):
        P = kc.P
        _lib.check(self.l.nic_gnn_alloc_bwd(P(out), P(on_hand), P(g_orders), P(sums), P(ratio), P(scale), P(d_out), P(g_on_hand), S, n_edges,
                                            e_self, e_sup, int(cap), B, ldb, self._s()))

    def groups_fwd(self, out, on_hand, orders, sums, ratio, scale, groups, order_row, cap, B, ldb):
        P = kc.P
        _lib.check(self.l.nic_gnn_alloc_groups_fwd(P(out), P(on_hand), on_hand.stride(0), P(orders), P(sums), P(ratio), P(scale), P(groups),
                                                   P(order_row), groups.shape[0], int(cap), B, ldb, self._s()))

    def groups_bwd(self, out, on_hand, g_orders, sums, ratio, scale, d_out, g_on_hand, groups, order_row, zero_first, zero_count, cap, B, ldb):
        P = kc.P
        _lib.check(self.l.nic_gnn_alloc_groups_bwd(P(out), P(on_hand), on_hand.stride(0), P(g_orders), P(sums), P(ratio), P(scale), P(d_out),
                                                   P(g_on_hand), P(groups), P(order_row), groups.shape[0], zero_first, zero_count, int(cap),
                                                   B, ldb, self._s()))

    @staticmethod
    def _order_tables(orders, S, ld):
        return Table(orders[:S].view(S, 1, -1), ld, 1, ld), Table(orders[S:], ld, 1)

    def env_fwd(self, prob, s, w, dem, orders, so, wo, reward):
        ts, tw = self._order_tables(orders, prob.S, prob.ldb)
        self.ops.env_step_fwd(prob, self.ops.EnvState(s, w), dem, ts, tw, None, self.ops.EnvState(so, wo), reward)

    def env_bwd(self, prob, s, w, dem, orders, gso, gwo, gr, gsi, gwi, g_orders):
        S = prob.S
        ts, tw = self._order_tables(orders, S, prob.ldb)
        self.ops.env_step_bwd(prob, self.ops.EnvState(s, w), dem, ts, tw, None, self.ops.EnvState(gso, gwo), gr, self.ops.EnvState(gsi, gwi),
                              (g_orders[:S].view(S, 1, -1), g_orders[S:], None))

    def alloc_env_fwd(self, prob, s, w, dem, out, orders, sums, ratio, scale, e_self, e_sup, cap, so, wo, reward):
        self.ops.gnn_alloc_env_fwd(prob, self.ops.EnvState(s, w), dem, out, orders, sums, ratio, scale, e_self, e_sup, cap,
                                   self.ops.EnvState(so, wo), reward)

    def alloc_env_bwd(self, prob, s, w, dem, out, orders, sums, ratio, scale, e_self, e_sup, cap, gso, gwo, gr, gsi, gwi, g_orders, d_out):
        self.ops.gnn_alloc_env_bwd(prob, self.ops.EnvState(s, w), dem, out, orders, sums, ratio, scale, e_self, e_sup, cap,
                                   self.ops.EnvState(gso, gwo), gr, self.ops.EnvState(gsi, gwi), g_orders, d_out)

    def round_orders(self, x, rows, B, ldb):
        _lib.check(self.l.nic_round_orders(kc.P(x), rows, B, ldb, self._s()))


# ==== backend 2: the float32 restatement on the CPU ===============================================================================
DEFECTS = {
    # defect -> the checkers whose tables must catch it
    "alloc_drops_the_last_batch_of_eight": ("alloc",),
    "alloc_leaves_the_self_loop_out_of_the_sum": ("alloc", "groups"),
    "clamp_passes_with_lt_instead_of_le": ("alloc", "groups", "data_driven"),
    "clamp_passes_the_gradient_above_one": ("alloc", "groups", "data_driven"),
    "relu_gradient_one_at_zero": ("data_driven",),
    "writes_one_padding_column": ("alloc", "segment_sum", "softplus", "round"),
    "leaves_a_d_out_row_unwritten": ("alloc", "groups"),
    "assigns_an_accumulated_gradient": ("alloc", "groups", "data_driven", "serial"),
    "segment_sum_skips_rows_past_32": ("segment_sum", "segment_sum_terms"),
    "terms_added_in_another_order": ("segment_sum_terms",),
    "rounds_half_away_from_zero": ("round",),
    "softplus_past_the_threshold_returns_z": ("softplus",),
    "softplus_log_of_one_plus_e": ("softplus",),
}


def _f32(x):
    return torch.tensor(x, dtype=torch.float32)


class TorchGlue:
    """Every kernel of the tables restated with float32 aten ops on the CPU, one lane's order of operations kept (serial sums in
    member order, separate multiplies and adds); writes into the same buffers through the same arguments.  `defect` breaks one
    thing on purpose."""
    device = "cpu"

    def __init__(self, defect=None):
        assert defect is None or defect in DEFECTS, defect
        self.defect = defect
        self._host = None

    def sync(self):
        pass

    def last_kernel(self):
        return None

    def _pad_defect(self, buf, B):
        if self.defect == "writes_one_padding_column" and buf.shape[-1] > B:
            buf[..., B] = 0.0

    # -- segment sums
    @staticmethod
    def _vec(dst, srcs, B, ldb):
        ok = ldb % 4 == 0 and dst.stride(0) % 4 == 0 and dst.data_ptr() % 16 == 0 and ceil4(B) <= ldb
        return ok and all(s.stride(0) % 4 == 0 and s.data_ptr() % 16 == 0 for s in srcs)

    def _segment(self, src, offsets, items, n, rows, cols):
        s = torch.zeros(rows, cols)
        if offsets is None:
            return s + src[:rows, n, :cols]
        for p in range(int(offsets[n]), int(offsets[n + 1])):
            s = s + src[:rows, int(items[p]), :cols]
        return s

    def segment_sum(self, dst, src, offsets, items, scale, R, n_dst, B, ldb, accumulate):
        self.segment_sum_terms(dst, [(src, offsets, items, scale)], R, n_dst, B, ldb, accumulate, _single=True)

    def segment_sum_terms(self, dst, terms, R, n_dst, B, ldb, accumulate, _single=False):
        cols = ceil4(B) if self._vec(dst, [t[0] for t in terms], B, ldb) else B
        rows = min(R, 32) if self.defect == "segment_sum_skips_rows_past_32" else R
        if self.defect == "terms_added_in_another_order" and not _single:
            terms = terms[::-1]
        for n in range(n_dst):
            y = dst[:rows, n, :cols].clone() if accumulate else None
            for src, offsets, items, scale in terms:
                v = self._segment(src, offsets, items, n, rows, cols)
                if scale is not None:
                    v = scale[n] * v
                else:
                    v = 1.0 * v
                y = v if y is None else y + v
            dst[:rows, n, :cols] = y
        if _single:
            self._pad_defect(dst, cols)

    # -- proportional allocation
    def _allocate(self, rows, self_row, oh, cap, batches=False):
        """serial float32 sum of the member rows (+ the self loop), ratio, scale"""
        members = list(rows)
        if batches and self.defect == "alloc_drops_the_last_batch_of_eight":
            members = members[:(len(members) - 1) // K_ALLOC_BATCH * K_ALLOC_BATCH]
        s = kc.serial_sum32(members) if members else torch.zeros_like(oh)
        if self_row is not None and self.defect != "alloc_leaves_the_self_loop_out_of_the_sum":
            s = s + self_row
        r = oh / (s + _f32(1e-10))
        return s, r, (torch.clamp(r, max=1.0) if cap else r)

    def _passes(self, r, cap):
        if not cap or self.defect == "clamp_passes_the_gradient_above_one":
            return torch.ones_like(r)
        return ((r < 1) if self.defect == "clamp_passes_with_lt_instead_of_le" else (r <= 1)).float()

    def _accumulate(self, buf, value):
        if self.defect == "assigns_an_accumulated_gradient":
            buf.copy_(value)
        else:
            buf.add_(value)

    def alloc_fwd(self, out, on_hand, orders, sums, ratio, scale, S, e_self, e_sup, cap, B, ldb):
        o = out[:, :B]
        s, r, sc = self._allocate([o[e] for e in range(S)], o[e_self] if e_self >= 0 else None, on_hand[:B], cap, batches=True)
        sums[:B], ratio[:B], scale[:B] = s, r, sc
        orders[:S, :B] = o[:S] * sc
        orders[S, :B] = o[e_sup]
        self._pad_defect(sums, B)

    def alloc_bwd(self, out, on_hand, g_orders, sums, ratio, scale, d_out, g_on_hand, S, n_edges, e_self, e_sup, cap, B, ldb):
        o, g = out[:, :B], g_orders[:, :B]
        dot = kc.serial_sum32([g[e] * o[e] for e in range(S)])
        d_scale = dot * self._passes(ratio[:B], cap)
        den = sums[:B] + _f32(1e-10)
        common = -(d_scale * on_hand[:B] / (den * den))
        g_sup = g[S].clone()
        last = n_edges - (1 if self.defect == "leaves_a_d_out_row_unwritten" else 0)
        for e in range(last):
            v = torch.zeros(B)
            if e < S or e == e_self:
                v = common.clone()
            if e < S:
                v = v + g[e] * scale[:B]
            if e == e_sup:
                v = g_sup
            d_out[e, :B] = v
        self._accumulate(g_on_hand[:B], d_scale / den)

    def groups_fwd(self, out, on_hand, orders, sums, ratio, scale, groups, order_row, cap, B, ldb):
        o = out[:, :B]
        for g, (first, count, e_self, e_sup) in enumerate(groups.tolist()):
            orders[int(order_row[e_sup]), :B] = o[e_sup]
            if count == 0 and e_self < 0:
                continue
            s, r, sc = self._allocate([o[first + i] for i in range(count)], o[e_self] if e_self >= 0 else None, on_hand[g, 0, :B], cap)
            sums[g, :B], ratio[g, :B], scale[g, :B] = s, r, sc
            for i in range(count):
                orders[int(order_row[first + i]), :B] = o[first + i] * sc

    def groups_bwd(self, out, on_hand, g_orders, sums, ratio, scale, d_out, g_on_hand, groups, order_row, zero_first, zero_count, cap, B, ldb):
        o = out[:, :B]
        skip = self.defect == "leaves_a_d_out_row_unwritten"
        for i in range(zero_count - (1 if skip else 0)):
            d_out[zero_first + i, :B] = 0.0
        for g, (first, count, e_self, e_sup) in enumerate(groups.tolist()):
            d_out[e_sup, :B] = g_orders[int(order_row[e_sup]), :B]
            if count == 0 and e_self < 0:
                continue
            gm = [g_orders[int(order_row[first + i]), :B] for i in range(count)]
            dot = kc.serial_sum32([gm[i] * o[first + i] for i in range(count)]) if count else torch.zeros(B)
            d_scale = dot * self._passes(ratio[g, :B], cap)
            den = sums[g, :B] + _f32(1e-10)
            common = -(d_scale * on_hand[g, 0, :B] / (den * den))
            for i in range(count):
                d_out[first + i, :B] = common + gm[i] * scale[g, :B]
            if e_self >= 0 and not (skip and zero_count == 0):
                d_out[e_self, :B] = common
            self._accumulate(g_on_hand[g, 0, :B], d_scale / den)

    # -- the env step around the allocation: the host build of the env-step bodies
    def _io(self, prob, s, w, dem, orders):
        if self._host is None:
            self._host = kc.HostSimBackend()
        ts, tw = HipGlue._order_tables(orders, prob.S, prob.ldb)
        return prob.make_io(s, w, None, dem, ts, tw, None), (ts, tw)

    def env_fwd(self, prob, s, w, dem, orders, so, wo, reward):
        io, _keep = self._io(prob, s, w, dem, orders)
        self._host.env_fwd(io, so, wo, None, reward)

    def env_bwd(self, prob, s, w, dem, orders, gso, gwo, gr, gsi, gwi, g_orders):
        io, _keep = self._io(prob, s, w, dem, orders)
        S = prob.S
        self._host.env_bwd(io, gso, gwo, None, gr.t2(), gsi, gwi, None, g_orders[:S], g_orders[S:], None)

    def alloc_env_fwd(self, prob, s, w, dem, out, orders, sums, ratio, scale, e_self, e_sup, cap, so, wo, reward):
        self.alloc_fwd(out, w[0, 0], orders, sums, ratio, scale, prob.S, e_self, e_sup, cap, prob.B, prob.ldb)
        self.env_fwd(prob, s, w, dem, orders, so, wo, reward)

    def alloc_env_bwd(self, prob, s, w, dem, out, orders, sums, ratio, scale, e_self, e_sup, cap, gso, gwo, gr, gsi, gwi, g_orders, d_out):
        self.env_bwd(prob, s, w, dem, orders, gso, gwo, gr, gsi, gwi, g_orders)
        self.alloc_bwd(out, w[0, 0], g_orders, sums, ratio, scale, d_out, gwi[0, 0], prob.S, d_out.shape[0], e_self, e_sup, cap, prob.B, prob.ldb)

    # -- order rounding
    def round_orders(self, x, rows, B, ldb):
        v = x[:rows, :B]
        if self.defect == "rounds_half_away_from_zero":
            x[:rows, :B] = torch.sign(v) * torch.floor(v.abs() + 0.5)
        else:
            x[:rows, :B] = torch.round(v)
        self._pad_defect(x, B)

    # -- the three elementwise heads (the entry points of kernel_checks' backends)
    def head_data_driven_fwd(self, Z, wh, mask, so, wo, S, Wn, Ww, B, ldb):
        z = Z[:, :B]
        if Wn == 0:
            so[:S, :B] = torch.relu(z[:S])
            return
        wo[:Wn, :B] = torch.relu(z[:Wn])
        a = torch.relu(z[Wn:]).reshape(S, Wn, B) * mask[:, :, None]
        for w in range(Wn):
            avail = kc.serial_sum32([wh[w, k, :B] for k in range(Ww)])
            _, _, sc = self._allocate([a[s, w] for s in range(S)], None, avail, True)
            so.view(S, Wn, ldb)[:, w, :B] = a[:, w] * sc

    def head_data_driven_bwd(self, Z, wh, mask, g_so, g_wo, dZ, g_wh, S, Wn, Ww, B, ldb):
        z = Z[:, :B]
        on = (z >= 0) if self.defect == "relu_gradient_one_at_zero" else (z > 0)
        if Wn == 0:
            dZ[:S, :B] = torch.where(on[:S], g_so[:S, :B], torch.zeros(()))
            return
        dZ[:Wn, :B] = torch.where(on[:Wn], g_wo[:Wn, :B], torch.zeros(()))
        a = torch.relu(z[Wn:]).reshape(S, Wn, B) * mask[:, :, None]
        gs = g_so[:, :B].reshape(S, Wn, B)
        for w in range(Wn):
            avail = kc.serial_sum32([wh[w, k, :B] for k in range(Ww)])
            s, r, sc = self._allocate([a[s_, w] for s_ in range(S)], None, avail, True)
            dot = kc.serial_sum32([gs[s_, w] * a[s_, w] for s_ in range(S)])
            d_scale = dot * self._passes(r, True)
            den = s + _f32(1e-10)
            common = -(d_scale * avail / (den * den))
            da = (gs[:, w] * sc + common) * mask[:, w, None]
            dZ[Wn:].view(S, Wn, ldb)[:, w, :B] = torch.where(on[Wn:].reshape(S, Wn, B)[:, w], da, torch.zeros(()))
            for k in range(Ww):
                self._accumulate(g_wh[w, k, :B], d_scale / den)

    @staticmethod
    def _sigmoid(x):
        return 1.0 / (1.0 + torch.exp(-x))

    def head_serial_fwd(self, Z, wh, ech, ub, so, wo, eo, E, Ww, We, B, ldb):
        up = [torch.full((B,), ub)] + [ech[j, 0, :B] for j in range(E)] + [wh[0, 0, :B]]
        for j in range(E + 2):
            a = self._sigmoid(Z[j, :B]) * up[j]
            (eo[j] if j < E else (wo[0] if j == E else so[0, 0]))[:B] = a

    def head_serial_bwd(self, Z, wh, ech, ub, gso, gwo, geo, dZ, gwi, gei, E, Ww, We, B, ldb):
        up = [torch.full((B,), ub)] + [ech[j, 0, :B] for j in range(E)] + [wh[0, 0, :B]]
        for j in range(E + 2):
            g = (geo[j] if j < E else (gwo[0] if j == E else gso[0]))[:B]
            sg = self._sigmoid(Z[j, :B])
            dZ[j, :B] = g * up[j] * sg * (1.0 - sg)
            if 1 <= j <= E:
                self._accumulate(gei[j - 1, 0, :B], g * sg)
            elif j == E + 1:
                self._accumulate(gwi[0, 0, :B], g * sg)

    def head_softplus_fwd(self, Z, o, rows, B, ldb):
        z = Z[:rows, :B]
        x = z + 1.0
        e = torch.exp(x)
        soft = torch.log(1.0 + e) if self.defect == "softplus_log_of_one_plus_e" else torch.log1p(e)
        o[:rows, :B] = torch.where(x > 20.0, z if self.defect == "softplus_past_the_threshold_returns_z" else x, soft)
        self._pad_defect(o, B)

    def head_softplus_bwd(self, Z, g, dZ, rows, B, ldb):
        x = Z[:rows, :B] + 1.0
        e = torch.exp(x)
        dZ[:rows, :B] = g[:rows, :B] * torch.where(x > 20.0, torch.ones(()), e / (e + 1.0))


CHECKERS = {
    "segment_sum": (SEG_CASES, check_segment_sum), "segment_sum_terms": (TERMS_CASES, check_segment_sum_terms),
    "alloc": (ALLOC_CASES, check_alloc), "groups": (GROUPS_CASES, check_alloc_groups), "alloc_env": (ALLOC_ENV_CASES, check_alloc_env),
    "round": (ROUND_CASES, check_round_orders), "data_driven": (kc.DATA_DRIVEN_CASES, kc.check_data_driven_head),
    "serial": (kc.SERIAL_CASES, kc.check_serial_head_case), "softplus": (kc.SOFTPLUS_CASES, kc.check_softplus_head_case),
}
