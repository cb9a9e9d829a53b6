"""Element-wise float64 check of the fused gather-MLP kernels (csrc/mlp3.hip) on the layouts the GNN engine hands them.

One case table (CASES), one checker (check_case), two backends - like kernel_checks.py and small_rollout_checks.py:
  * HipMlp3      - ops.mlp3_desc / mlp3_fwd / mlp3_bwd_hist / mlp3_bwd_fused / wgrad_reduce on the device (tests/test_gpu_mlp3.py);
  * EmulatedMlp3 - a float32 torch-CPU restatement that writes into the same buffers through the address formulas documented in
                   include/nic_rollout.h, with a `defect=` switch that restates one class of kernel error each
                   (tests/test_mlp3_checks_host.py: the clean emulation passes every case, every defect fails at least one -
                   the proof that the checker would notice, without ever running a broken kernel on a device).
The checker never uses the emulation's address arithmetic: it un-permutes the buffers with views (native history =
[E * ldb / 32][32][32] blocks, block e * ldb / 32 + chunk; strided = period t's slice of [rows][T][E][ldb]).

What a case checks
  * Y, H1, H2, dX and the reduced dW / db of all three layers against float64 torch autograd on the densely gathered input,
    element-wise:  |got - want| <= C * scale + A.
  * X_hist == the gathered input, Ysum == Y + residual: bit for bit.
  * The gradient reduced after one backward launch (scale 1) == the gradient reduced after a second launch into the same slabs
    (scale 0.5): bit for bit (slabs accumulate; doubling and halving are exact).
  * Every element the launch does not own is pre-filled with SENT and must come back unchanged: the columns past B of every row,
    the entity rows n_live .. n_ent - 1 of Y / Ysum / dX (and of the histories), the other periods' slices of the histories, the
    slab columns past the bias column (zero).
  * The kernel variant the launcher noted (nic_last_kernel) is the one expected_kernels() derives from the case.

scale: per element, the contraction that produces it with the absolute value of every factor (float64 factors), as `_close` of
  tests/test_gpu_kernels.py takes it for one GEMM:
    H1: |W1| |x| + |b1|     H2: |W2| |h1| + |b2|     Y: |W3| |h2| + |b3| + |y|
    dX: |W1|^T |dz1|        dW_l: |dz_l| |a_(l-1)|^T  (a_0 = x, a_1 = h1, a_2 = h2)        db_l: sum over columns of |dz_l|
  (dz_l = the gradient at layer l's pre-activation).  The error an element inherits from the layers before it is not in its own
  contraction; it is in the measured constant:
C, A: A = 1e-6 as in `_close`.  C is not chosen from what the kernels give: the same MLP was run in float32 with plain torch
  CPU ops (Problem.float32_ratios) on every case of the table and the largest err / scale against float64 taken:
    Y 4.0e-07  H1 3.5e-07  H2 3.7e-07  dX 7.7e-07  dW1 2.9e-06  db1 4.0e-07  dW2 3.2e-06  db2 1.9e-07  dW3 1.7e-06  db3 2.2e-07
  (the weight gradients' figures come from the B = 1 cases: one product per element, whose dz factor carries the cancellation of
  the layers behind it).  C = 8 x the largest = 8 x 3.2e-06 = 2.56e-05, above the project's GEMM band of 4e-6; the 8 covers the
  kernels' different but equally valid summation order: MFMA 4 x 4 blocks, per-wavefront partial sums, slab reduce.
  tests/test_mlp3_checks_host.py measures the ratios again and fails if the recorded figure is off by more than a factor 2.

Dispatch cells the table reaches (test_the_table_reaches_every_dispatch_cell):
  mlp3_fwd_kernel<KS,CH,ADDR>: KS 4 / 16 / 33 / 48, CH 1 and 2, ADDR 1 (kAddrBuf) and 2 (kAddrBufX); ADDR 0 (kAddrFlat) needs
    rows 2 GiB apart and stays with test_mlp3_fwd_with_rows_too_far_apart_for_32_bit_offsets;
  mlp3_bwd_hist_kernel<1|2|3,stored|gather> and <1|2,stored|gather,tail>: every instantiation of the launcher;
  mlp3_bwd_fused_kernel<1|2|3>.
"""
import zlib
from collections import namedtuple
from functools import lru_cache

import torch
import torch.nn.functional as F

F32_WORST = 3.2e-6     # largest err / scale of plain float32 torch against float64 over the table (module docstring)
C_BAND, A_BAND = max(8 * F32_WORST, 4e-6), 1e-6
SENT = -1234.5     # finite: the backward reads the dead columns of H1 / H2 (and multiplies them by a zero gradient)
FWD_PAIR_MIN_WAVES, FWD_SLOTS = 2048, 256 * 4 * 5     # csrc/mlp3.hip: kFwdPairMinWaves, kFwdSlots
HIST_BLOCKS, WAVES_PER_BLOCK = 512, 4                  # kHistBlocks / kFusedBlocks, kHistWaves / kFusedWaves

Seg = namedtuple("Seg", "kind rows n_src")   # kind: "id" (identity map) | "map" (random, with -1) | "const" | "bcast"
Case = namedtuple("Case", "id segs n_out act E_live E_buf B hist x_hist residual")
# hist: "default" | "native" | ("strided", T, t);  x_hist: "stored" | "gather";  act: 0 none / 1 ELU / 2 softplus


def pad32(n):
    return (n + 31) // 32 * 32


def _mlp3_reference(x, W, act):
    """x: (cols, K) float64; W: [(w1, b1), (w2, b2), (w3, b3)] float64 with requires_grad."""
    h1 = F.elu(F.linear(x, *W[0]))
    h2 = F.elu(F.linear(h1, *W[1]))
    z = F.linear(h2, *W[2])
    y = F.elu(z) if act == 1 else (F.softplus(z) if act == 2 else z)
    return y, h1, h2


# ---- the case table ---------------------------------------------------------------------------------------------------------

def _segs(spec, n_src=4):
    """(32, "m32", "c1", "b5") -> identity 32 rows, mapped 32 rows, per-entity constant 1 row, broadcast source 5 rows"""
    out = []
    for s in spec:
        if isinstance(s, int):
            out.append(Seg("id", s, 0))
        else:
            out.append(Seg({"m": "map", "c": "const", "b": "bcast"}[s[0]], int(s[1:]), n_src))
    return tuple(out)


def _case(cid, spec, n_out=32, act=1, E=3, E_buf=None, B=33, hist="default", x_hist=None, residual=False):
    x_hist = x_hist or ("gather" if hist == "native" else "stored")
    return Case(cid, _segs(spec), n_out, act, E, E_buf or E, B, hist, x_hist, residual)


def _table():
    t = []
    # native history (the engine's default): forward CH = 1 + gather backward, at every scenario-count edge; the per-entity
    # constant last behind two gathered 32-row segments (ragged last chunk at B = 33, 70; ldb / 32 odd at B = 70)
    for B in (1, 31, 32, 33, 64, 70):
        t.append(_case(f"native-K65-B{B}", (32, "m32", "c1"), B=B, hist="native"))
        t.append(_case(f"native-K7-B{B}", (7,), B=B, hist="native"))
    # forward pair variant (CH = 2) with native history and an odd chunk count; 2193 and 4386 items over the backward kernels'
    # 2048 persistent wavefronts: some walk 1, 2 or 3 items, and every workgroup reduces four busy wavefronts
    for E in (17, 34):
        t.append(_case(f"items-E{E}-native-K65", (32, "m32", "c1"), E=E, B=4096 + 20, hist="native"))
        t.append(_case(f"items-E{E}-stored-K96", (32, "m32", "m32"), E=E, B=4096 + 20))
    t.append(_case("items-E17-native-K96", (32, "m32", "m32"), E=17, B=4096 + 20, hist="native"))
    # ent_row_stride: the first 5 entities of buffers that hold 9 (edge update: n_out = 32 with the residual folded in; output
    # MLP: n_out = 1 softplus), under each backward kernel
    for B in (70, 33):
        for hist in ("native", "default"):
            t.append(_case(f"live5of9-edge-{hist}-B{B}", (32, "m32", "m32"), E=5, E_buf=9, B=B, hist=hist, residual=True))
            t.append(_case(f"live5of9-out-{hist}-B{B}", (32,), n_out=1, act=2, E=5, E_buf=9, B=B, hist=hist))
    t.append(_case("live5of9-edge-noresidual-B70", (32, "m32", "m32"), E=5, E_buf=9, B=70, hist="default", x_hist="gather"))
    # hist_row_stride: period 1 of 3 interleaved in one row
    for name, spec in (("K33", (20, "m13")), ("K65", (32, "m32", "c1"))):
        for xh in ("stored", "gather"):
            t.append(_case(f"period1of3-{name}-{xh}", spec, E=4, B=70, hist=("strided", 3, 1), x_hist=xh))
    # every (kg, tail) cell of the history backward, stored and gather; the forward's K tiers at their edges
    ks = {33: (32, "c1"), 34: (32, "m2"), 50: (20, "m30"), 64: (32, "m32"), 65: ("m32", 32, "c1"), 66: (32, "m32", "m2"),
          80: (32, "m32", 16), 95: (32, "m32", "m31"), 96: (32, "m32", "m32")}
    for K, spec in ks.items():
        for xh in ("stored", "gather"):
            t.append(_case(f"K{K}-{xh}", spec, B=33, x_hist=xh))
    for K, spec in ((1, (1,)), (8, ("m8",)), (9, (4, "m5")), (32, ("m32",)), (67, (32, "m32", 3))):
        t.append(_case(f"K{K}-tier", spec, B=40, hist="native" if K in (8, 32) else "default"))
    # n_out 1..32 under every output activation
    for n_out in (1, 5, 8, 12, 20, 31, 32):
        for act in (0, 1, 2):
            t.append(_case(f"nout{n_out}-act{act}", (7, "m6"), n_out=n_out, act=act, E=2, B=37,
                           hist="native" if n_out in (5, 20) else "default"))
    # segment forms: four segments (the maximum) with -1 entries in two maps and the constant last; a broadcast source
    t.append(_case("segs4-stored", (8, "m8", "m8", "c1"), E=6, B=33))
    t.append(_case("segs4-native", (8, "m8", "m8", "c1"), E=6, B=33, hist="native"))
    t.append(_case("bcast-stored", ("b5", 6), E=4, B=33))
    t.append(_case("bcast-native", ("b5", 6, "c1"), E=4, B=70, hist="native"))
    assert len({c.id for c in t}) == len(t)
    return t


CASES = _table()
BY_ID = {c.id: c for c in CASES}


def expected_kernels(case):
    """The variants the launchers of csrc/mlp3.hip pick for a case: (forward, history backward, history-free backward)."""
    K = sum(s.rows for s in case.segs)
    ks = (K + 1) // 2
    tier = 4 if ks <= 4 else (16 if ks <= 16 else (33 if ks <= 33 else 48))
    waves = case.E_live * ((case.B + 31) // 32)
    ch = 2 if FWD_PAIR_MIN_WAVES <= waves <= FWD_SLOTS else 1
    kg, tail = (K + 31) // 32, ""
    if K >= 32 and K % 32 == 1:
        kg, tail = K // 32, ",tail"
    return (f"mlp3_fwd_kernel<{tier},{ch},{2 if case.x_hist == 'stored' else 1}>",
            f"mlp3_bwd_hist_kernel<{kg},{case.x_hist}{tail}>", f"mlp3_bwd_fused_kernel<{(K + 31) // 32}>")


# ---- a case's data and its float64 reference ---------------------------------------------------------------------------------

class Problem:
    """Sources, maps, weights, dY, residual of a case (CPU, float32) and the float64 reference of everything the kernels write."""

    def __init__(self, case):
        self.case = c = case
        gen = torch.Generator().manual_seed(zlib.crc32(c.id.encode()))
        E, Eb, B = c.E_live, c.E_buf, c.B
        self.ld = ld = pad32(B)
        self.K = K = sum(s.rows for s in c.segs)
        self.sources, dense = [], []     # (tensor, int32 map or None, per_scenario)
        for si, s in enumerate(c.segs):
            if s.kind == "const":        # per-entity constant (an edge's lead time): [rows][entities]
                t = torch.randn(s.rows, Eb, generator=gen)
                self.sources.append((t, None, False))
                dense.append(t[:, :E, None].expand(s.rows, E, B))
                continue
            n = {"id": Eb, "map": s.n_src, "bcast": 1}[s.kind]
            t = torch.zeros(s.rows, n, ld)      # padding columns zero: what the gather backward asks of its sources
            t[:, :, :B] = torch.randn(s.rows, n, B, generator=gen)
            idx = None
            if s.kind == "map":
                idx = torch.randint(-1, n, (Eb,), generator=gen, dtype=torch.int32)
                idx[si % E] = -1                # every map has a virtual (all-zero) node ...
                idx[(si + 1) % E] = si % n      # ... and, from two entities on, a real one
                dense.append(torch.where((idx[:E] >= 0)[None, :, None], t[:, idx[:E].clamp_min(0).long(), :B], torch.zeros(())))
            elif s.kind == "bcast":
                dense.append(t[:, :, :B].expand(s.rows, E, B))
            else:
                dense.append(t[:, :E, :B])
            self.sources.append((t, idx, True))
        self.X = torch.cat(dense, dim=0).contiguous()     # [K][E][B]
        self.dims = dims = [(32, K), (32, 32), (c.n_out, 32)]
        self.W = [(torch.randn(n, k, generator=gen) / k ** 0.5, torch.randn(n, generator=gen) * 0.3) for n, k in dims]
        self.gY = torch.zeros(c.n_out, Eb, ld)
        self.gY[:, :E, :B] = torch.randn(c.n_out, E, B, generator=gen)
        self.R = None
        if c.residual:
            self.R = torch.zeros(c.n_out, Eb, ld)
            self.R[:, :E, :B] = torch.randn(c.n_out, E, B, generator=gen)
        self.ref = self._reference(torch.float64)
        self.scale = self._scales()

    def _cols(self, t):      # [rows][E][B] -> (E * B, rows)
        return t.permute(1, 2, 0).reshape(self.case.E_live * self.case.B, t.shape[0])

    def _rows(self, t):      # (E * B, rows) -> [rows][E][B]
        return t.reshape(self.case.E_live, self.case.B, t.shape[1]).permute(2, 0, 1)

    def _reference(self, dtype):
        c = self.case
        W = [(w.to(dtype).requires_grad_(True), b.to(dtype).requires_grad_(True)) for w, b in self.W]
        x = self._cols(self.X).to(dtype).requires_grad_(True)
        y, h1, h2 = _mlp3_reference(x, W, c.act)
        (y * self._cols(self.gY[:, :c.E_live, :c.B]).to(dtype)).sum().backward()
        out = {"Y": self._rows(y.detach()), "H1": self._rows(h1.detach()), "H2": self._rows(h2.detach()), "dX": self._rows(x.grad)}
        for l, (w, b) in enumerate(W, 1):
            out[f"dW{l}"], out[f"db{l}"] = w.grad, b.grad
        return out

    def _scales(self):
        """Per element, the contraction that produces it with the absolute value of every factor (float64 factors)."""
        c = self.case
        (w1, b1), (w2, b2), (w3, b3) = [(w.double(), b.double()) for w, b in self.W]
        x, gy = self._cols(self.X).double(), self._cols(self.gY[:, :c.E_live, :c.B]).double()
        h1, h2, y = (self._cols(self.ref[k]) for k in ("H1", "H2", "Y"))
        elu_grad = lambda h: torch.where(h > 0, torch.ones((), dtype=h.dtype), h + 1)  # noqa: E731
        dz3 = gy * (elu_grad(y) if c.act == 1 else (1 - torch.exp(-y) if c.act == 2 else torch.ones_like(y)))
        dz2 = (dz3 @ w3) * elu_grad(h2)
        dz1 = (dz2 @ w2) * elu_grad(h1)
        out = {"H1": self._rows(x.abs() @ w1.abs().t() + b1.abs()), "H2": self._rows(h1.abs() @ w2.abs().t() + b2.abs()),
               "Y": self._rows(h2.abs() @ w3.abs().t() + b3.abs() + y.abs()), "dX": self._rows(dz1.abs() @ w1.abs())}
        for l, (dz, a) in enumerate(((dz1, x), (dz2, h1), (dz3, h2)), 1):
            out[f"dW{l}"], out[f"db{l}"] = dz.abs().t() @ a.abs(), dz.abs().sum(dim=0)
        return out

    def float32_ratios(self):
        """Largest err / scale of the same MLP in float32 (plain torch CPU ops) against float64, per checked quantity."""
        got = self._reference(torch.float32)
        return {k: float(((got[k].double() - self.ref[k]).abs() / self.scale[k]).max()) for k in self.ref}


@lru_cache(maxsize=2)
def problem(case):
    return Problem(case)


# ---- the buffers of one run, pre-filled with the sentinel ----------------------------------------------------------------------

class Hist:
    """One history buffer: `full` is the whole allocation (every period), `base` the flat view from period t's origin that the
    launch gets, `stride` the descriptor's hist_row_stride."""

    def __init__(self, case, rows, ld, device):
        Eb = self.Eb = case.E_buf
        self.ld = ld
        self.T, self.t = (case.hist[1], case.hist[2]) if isinstance(case.hist, tuple) else ((3, 1) if case.hist == "native" else (1, 0))
        self.native, self.rows = case.hist == "native", rows
        if self.native:      # the engine's [period][entity x chunk][32 rows][32 scenarios]
            self.full = torch.full((self.T, 32 * Eb * ld), SENT, device=device)
            origin = self.t * 32 * Eb * ld
        else:
            self.full = torch.full((rows, self.T, Eb, ld), SENT, device=device)
            origin = self.t * Eb * ld
        self.base = self.full.view(-1)[origin:]
        # (the engine hands the native layout its period stride too; the kernels ignore it there)
        self.stride = self.T * Eb * ld if (self.T > 1 or self.native) else 0

    def dense(self):
        """-> ([rows][E_buf][ld] view of period t on the CPU, the other periods)"""
        full = self.full.cpu()
        if self.native:
            cur = full[self.t].view(self.Eb, self.ld // 32, 32, 32).permute(2, 0, 1, 3).reshape(32, self.Eb, self.ld)
            rest = torch.cat([full[:self.t], full[self.t + 1:]])
        else:
            cur = full[:, self.t]
            rest = torch.cat([full[:, :self.t], full[:, self.t + 1:]], dim=1)
        return cur, rest


class Buffers:
    def __init__(self, prob, device, hist_slots, fused_slots):
        c, ld = prob.case, prob.ld
        self.device = device
        ent = lambda rows: torch.full((rows, c.E_buf, ld), SENT, device=device)  # noqa: E731
        self.ent_row_stride = c.E_buf * ld if c.E_buf != c.E_live else 0
        self.Y = ent(c.n_out)
        self.Ysum = ent(c.n_out) if c.residual else None
        self.dX = {"hist": ent(prob.K), "fused": ent(prob.K)}
        self.H1, self.H2 = Hist(c, 32, ld, device), Hist(c, 32, ld, device)
        self.Xh = Hist(c, prob.K, ld, device) if c.x_hist == "stored" else None
        self.hist_row_stride, self.native = self.H1.stride, self.H1.native
        lds = lambda k: (k + 1 + 3) // 4 * 4  # noqa: E731
        self.slabs = {"hist": [torch.zeros(hist_slots, n, lds(k), device=device) for n, k in prob.dims],
                      "fused": [torch.zeros(fused_slots, n, lds(k), device=device) for n, k in prob.dims]}
        dv = lambda t: None if t is None else t.to(device)  # noqa: E731
        self.sources = [(dv(t), dv(idx), ps) for t, idx, ps in prob.sources]
        self.gY, self.R = dv(prob.gY), dv(prob.R)
        self.packed = torch.cat([t.reshape(-1) for wb in prob.W for t in wb]).to(device)
        (w1, b1), (w2, b2), (w3, b3) = prob.W        # (ops.mlp3_pack_transposed, restated: the host run has no device)
        w3t, b3p = torch.zeros(32, 32), torch.zeros(32)
        w3t[:, :c.n_out], b3p[:c.n_out] = w3.t(), b3
        self.packed_t = torch.cat([w1.t().reshape(-1), b1, w2.t().reshape(-1), b2, w3t.reshape(-1), b3p]).to(device)


# ---- the checker -------------------------------------------------------------------------------------------------------------

def _band(got, want, scale, what, figures):
    err = (got.double() - want).abs()
    bound = C_BAND * scale + A_BAND
    figures[what[-1]] = max(figures.get(what[-1], 0.0), float((err / bound).max()))
    bad = err > bound
    assert not bool(bad.any()), (what, "err / bound", float((err / bound).max()), "elements outside", int(bad.sum()))


def _region(dense, case, want, scale, what, figures, rest=None):
    """dense: [rows][E_buf][ld] (CPU).  Its live part [:, :E_live, :B] against `want` (bit-equal when scale is None, inside the
    band otherwise); every other element, and all of `rest`, still the sentinel."""
    assert dense.shape[0] == want.shape[0], (what, dense.shape, want.shape)
    live = dense[:, :case.E_live, :case.B]
    if scale is None:
        assert torch.equal(live, want), (what, "not bit-equal", int((live != want).sum()))
    else:
        _band(live, want, scale, what, figures)
    dead = dense.clone()
    dead[:, :case.E_live, :case.B] = SENT
    assert bool((dead == SENT).all()), (what, "elements outside the live region overwritten", int((dead != SENT).sum()))
    if rest is not None:
        assert bool((rest == SENT).all()), (what, "another period's slice overwritten", int((rest != SENT).sum()))


def check_case(case, backend, prob=None):
    """Run `case` through `backend` and check everything the module docstring lists.  Returns {quantity: worst err / bound}."""
    prob = prob or problem(case)
    buf = Buffers(prob, backend.device, backend.hist_slots(), backend.fused_slots())
    ref, scale, figures = prob.ref, prob.scale, {}
    want_fwd, want_hist, want_fused = expected_kernels(case)

    def kernel_is(want):
        got = backend.last_kernel()
        assert got is None or got == want, (case.id, got, want)

    backend.fwd(prob, buf)
    kernel_is(want_fwd)
    for name, h in (("H1", buf.H1), ("H2", buf.H2)):
        cur, rest = h.dense()
        _region(cur, case, ref[name], scale[name], (case.id, name), figures, rest)
    if buf.Xh is not None:
        cur, rest = buf.Xh.dense()
        _region(cur, case, prob.X, None, (case.id, "X_hist"), figures, rest)
    Y = buf.Y.cpu()
    _region(Y, case, ref["Y"], scale["Y"], (case.id, "Y"), figures)
    if case.residual:
        want = (Y + prob.R)[:, :case.E_live, :case.B]     # the same float32 add: bit for bit
        _region(buf.Ysum.cpu(), case, want, None, (case.id, "Ysum"), figures)

    for mode, want_kernel in (("hist", want_hist), ("fused", want_fused)):
        backend.bwd(prob, buf, mode)
        kernel_is(want_kernel)
        once = backend.reduce(prob, buf, mode, 1.0)
        backend.bwd(prob, buf, mode)
        twice = backend.reduce(prob, buf, mode, 0.5)
        _region(buf.dX[mode].cpu(), case, ref["dX"], scale["dX"], (case.id, mode, "dX"), figures)
        for l, ((gw1, gb1), (gw2, gb2)) in enumerate(zip(once, twice), 1):
            assert torch.equal(gw1, gw2) and torch.equal(gb1, gb2), (case.id, mode, l, "two launches are not twice one launch")
            _band(gw2, ref[f"dW{l}"], scale[f"dW{l}"], (case.id, mode, f"dW{l}"), figures)
            _band(gb2, ref[f"db{l}"], scale[f"db{l}"], (case.id, mode, f"db{l}"), figures)
        for sl, (n, k) in zip(buf.slabs[mode], prob.dims):
            assert float(sl[:, :, k + 1:].abs().sum()) == 0.0, (case.id, mode, "slab columns past the bias column written")
    # the inputs of the launches are theirs to read only
    for (t, idx, _), (t0, idx0, _) in zip(buf.sources, prob.sources):
        assert torch.equal(t.cpu(), t0) and (idx is None or torch.equal(idx.cpu(), idx0)), (case.id, "a source buffer was written")
    return figures


# ---- backend 1: the HIP kernels ----------------------------------------------------------------------------------------------

class HipMlp3:
    device = "cuda"

    def __init__(self):
        from neural_inventory_control_amd import _lib, ops
        _lib.require_device()
        self.ops, self._lib = ops, _lib

    def hist_slots(self):
        return self.ops.mlp3_bwd_hist_slots()

    def fused_slots(self):
        return self.ops.mlp3_bwd_fused_slots()

    def last_kernel(self):
        return self._lib.lib().nic_last_kernel().decode()

    def desc(self, prob, buf):
        c, ops = prob.case, self.ops
        segs = [ops.Mlp3Segment(t, idx, per_scenario=ps) for t, idx, ps in buf.sources]
        return ops.mlp3_desc(segs, buf.packed, c.E_live, c.B, prob.ld, c.n_out, c.act, buf.hist_row_stride, buf.packed_t,
                             hist_native=buf.native, ent_row_stride=buf.ent_row_stride)

    def fwd(self, prob, buf):
        self.ops.mlp3_fwd(self.desc(prob, buf), buf.Y, buf.Xh.base if buf.Xh is not None else None, buf.H1.base, buf.H2.base,
                          buf.R, buf.Ysum)
        torch.cuda.synchronize()

    def bwd(self, prob, buf, mode):
        d = self.desc(prob, buf)
        if mode == "hist":
            self.ops.mlp3_bwd_hist(d, buf.gY, buf.Y, buf.Xh.base if buf.Xh is not None else None, buf.H1.base, buf.H2.base,
                                   buf.dX[mode], buf.slabs[mode])
        else:
            self.ops.mlp3_bwd_fused(d, buf.gY, buf.Y, buf.dX[mode], buf.slabs[mode])
        torch.cuda.synchronize()

    def reduce(self, prob, buf, mode, scale):
        out = []
        for sl, (n, k) in zip(buf.slabs[mode], prob.dims):
            gw, gb = torch.zeros(n, k, device=self.device), torch.zeros(n, device=self.device)
            self.ops.wgrad_reduce(sl, gw, gb, k, scale)
            torch.cuda.synchronize()
            out.append((gw.cpu(), gb.cpu()))
        return out


# ---- backend 2: the float32 restatement on the CPU ---------------------------------------------------------------------------

DEFECTS = ("native_ignores_chunk", "native_block_uses_E_not_ldb", "ent_stride_ignored", "hist_stride_ignored",
           "resets_grads_per_item", "const_row_leaks_into_dead_columns", "writes_skipped_entities",
           "w3_rows_past_n_out_not_masked")


def _elu_grad_from_out(h):
    return torch.where(h > 0, torch.ones(()), h + 1)


class EmulatedMlp3:
    """The launches of csrc/mlp3.hip restated with float32 torch ops on flat buffers: every load and store goes through the
    address formulas of include/nic_rollout.h (`_ent_addr`, `_hist_addr`, `_gather`), the backward walks (entity, 32-scenario
    chunk) items over 2048 persistent wavefronts like the kernels and adds each workgroup's (history backward) or wavefront's
    (history-free backward) sum to its slab slot.  `defect` breaks one of these on purpose."""
    device = "cpu"

    def __init__(self, defect=None):
        assert defect is None or defect in DEFECTS, defect
        self.defect = defect

    def hist_slots(self):
        return HIST_BLOCKS

    def fused_slots(self):
        return HIST_BLOCKS * WAVES_PER_BLOCK

    def last_kernel(self):
        return None

    # -- addressing
    def _geometry(self, prob, buf):
        c, ld = prob.case, prob.ld
        ent_ld = buf.ent_row_stride if buf.ent_row_stride and self.defect != "ent_stride_ignored" else c.E_live * ld
        hs = buf.hist_row_stride if buf.hist_row_stride and self.defect != "hist_stride_ignored" else ent_ld
        chunks = (c.B + 31) // 32
        return ent_ld, hs, chunks

    def _ent_addr(self, prob, buf, rows, n_ent, n_col):
        """element offsets [rows][n_ent][n_col] of row * ent_row_stride + e * ldb + b"""
        ent_ld, _, _ = self._geometry(prob, buf)
        r, e, b = torch.arange(rows)[:, None, None], torch.arange(n_ent)[None, :, None], torch.arange(n_col)[None, None, :]
        return r * ent_ld + e * prob.ld + b

    def _hist_addr(self, prob, buf, rows, n_col):
        c, ld = prob.case, prob.ld
        _, hs, _ = self._geometry(prob, buf)
        r, e, b = torch.arange(rows)[:, None, None], torch.arange(c.E_live)[None, :, None], torch.arange(n_col)[None, None, :]
        if not buf.native:
            return r * hs + e * ld + b
        chunk = b // 32
        if self.defect == "native_ignores_chunk":
            chunk = chunk * 0
        per_entity = c.E_live if self.defect == "native_block_uses_E_not_ldb" else ld // 32
        return ((e * per_entity + chunk) * 32 + r) * 32 + b % 32

    @staticmethod
    def _store(flat, addr, values, what):
        flat = flat.view(-1) if flat.dim() != 1 else flat
        assert int(addr.min()) >= 0 and int(addr.max()) < flat.numel(), (what, "a store outside the buffer")
        flat[addr.reshape(-1)] = values.reshape(-1)

    @staticmethod
    def _load(flat, addr, what):
        flat = flat.view(-1) if flat.dim() != 1 else flat
        assert int(addr.min()) >= 0 and int(addr.max()) < flat.numel(), (what, "a load outside the buffer")
        return flat[addr.reshape(-1)].reshape(addr.shape)

    def _gather(self, prob, buf, n_col):
        """the K input rows of every entity, columns 0 .. n_col - 1 (whole chunks: the row-owner reads of the backward take the
        dead columns of the last chunk too):  seg.base[r * row_stride + ent * ent_stride + b * scn_stride], ent < 0 reads 0"""
        c, parts = prob.case, []
        for t, idx, per_scenario in buf.sources:
            rows = t.shape[0]
            ent = idx[:c.E_live].long() if idx is not None else torch.arange(c.E_live)
            row_stride, ent_stride, scn = t.stride(0), (t.stride(1) if t.shape[1] > 1 else 0), (1 if per_scenario else 0)
            r, b = torch.arange(rows)[:, None, None], torch.arange(n_col)[None, None, :]
            addr = r * row_stride + ent.clamp_min(0)[None, :, None] * ent_stride + b * scn
            v = self._load(t, addr, "gather")
            parts.append(torch.where((ent >= 0)[None, :, None], v, torch.zeros(())))
        return torch.cat(parts, dim=0)      # [K][E][n_col]

    def _weights(self, prob, buf):
        p, o = buf.packed, 0
        out = []
        for n, k in prob.dims:
            out.append((p[o:o + n * k].view(n, k), p[o + n * k:o + n * k + n]))
            o += n * k + n
        return out

    def _mlp(self, prob, buf, x):      # x [K][E][cols] -> h1, h2, y
        c = prob.case
        (w1, b1), (w2, b2), (w3, b3) = self._weights(prob, buf)
        cols = x.reshape(prob.K, -1)
        h1 = F.elu(w1 @ cols + b1[:, None])
        h2 = F.elu(w2 @ h1 + b2[:, None])
        z = w3 @ h2 + b3[:, None]
        y = F.elu(z) if c.act == 1 else (torch.where(z > 20, z, torch.log1p(torch.exp(z))) if c.act == 2 else z)
        shape = lambda t: t.reshape(t.shape[0], x.shape[1], x.shape[2])  # noqa: E731
        return shape(h1), shape(h2), shape(y)

    # -- launches
    def fwd(self, prob, buf):
        c = prob.case
        x = self._gather(prob, buf, c.B)
        h1, h2, y = self._mlp(prob, buf, x)
        ha = self._hist_addr(prob, buf, 32, c.B)
        self._store(buf.H1.base, ha, h1, "H1")
        self._store(buf.H2.base, ha, h2, "H2")
        if buf.Xh is not None:
            self._store(buf.Xh.base, self._hist_addr(prob, buf, prob.K, c.B), x, "X_hist")
        ya = self._ent_addr(prob, buf, c.n_out, c.E_live, c.B)
        self._store(buf.Y, ya, y, "Y")
        if buf.Ysum is not None:
            self._store(buf.Ysum, ya, self._load(buf.R, ya, "residual") + y, "Ysum")
        if self.defect == "writes_skipped_entities" and c.E_buf > c.E_live:
            extra = self._ent_addr(prob, buf, c.n_out, c.E_buf, c.B)[:, c.E_live:]
            self._store(buf.Y, extra, torch.zeros(extra.shape), "Y of the skipped entities")

    def bwd(self, prob, buf, mode):
        c, K, E = prob.case, prob.K, prob.case.E_live
        _, _, chunks = self._geometry(prob, buf)
        n_col = chunks * 32
        live = (torch.arange(n_col) < c.B)[None, None, :]
        (w1, b1), (w2, b2), (w3, b3) = self._weights(prob, buf)
        ya = self._ent_addr(prob, buf, c.n_out, E, n_col)
        gy, yo = self._load(buf.gY, ya, "dY"), self._load(buf.Y, ya, "Y")
        if mode == "hist":       # stored activations (dead columns of the last chunk included: what the buffer holds)
            ha = self._hist_addr(prob, buf, 32, n_col)
            h1, h2 = self._load(buf.H1.base, ha, "H1"), self._load(buf.H2.base, ha, "H2")
            x = (self._load(buf.Xh.base, self._hist_addr(prob, buf, K, n_col), "X_hist") if buf.Xh is not None
                 else self._gather(prob, buf, n_col))
        else:                    # gathered again, hidden layers recomputed
            x = self._gather(prob, buf, n_col)
            h1, h2, _ = self._mlp(prob, buf, x)
        act_grad = _elu_grad_from_out(yo) if c.act == 1 else (1 - torch.exp(-yo) if c.act == 2 else torch.ones_like(yo))
        dz3 = torch.zeros(32, E, n_col)
        dz3[:c.n_out] = torch.where(live, gy * act_grad, torch.zeros(()))
        w3p = torch.zeros(32, 32)
        w3p[:c.n_out] = w3
        if self.defect == "w3_rows_past_n_out_not_masked" and c.n_out < 32:
            dz3[c.n_out:] = dz3[:1]        # lanes whose row does not exist read row 0 of their column ...
            w3p[c.n_out:] = 0.5            # ... and whatever follows W3 in the packed weights
        flat = lambda t: t.reshape(t.shape[0], -1)  # noqa: E731
        dz2 = (w3p.t() @ flat(dz3)).reshape(32, E, n_col) * _elu_grad_from_out(h2)
        dz1 = (w2.t() @ flat(dz2)).reshape(32, E, n_col) * _elu_grad_from_out(h1)
        if self.defect == "w3_rows_past_n_out_not_masked":
            dz3 = dz3.clone()
            dz3[c.n_out:] = 0
        dz2, dz1 = torch.where(live, dz2, torch.zeros(())), torch.where(live, dz1, torch.zeros(()))
        dx = (w1.t() @ flat(dz1)).reshape(K, E, n_col)
        xa = self._ent_addr(prob, buf, K, E, c.B)
        self._store(buf.dX[mode], xa, dx[:, :, :c.B], "dX")
        if self.defect == "writes_skipped_entities" and c.E_buf > E:
            extra = self._ent_addr(prob, buf, K, c.E_buf, c.B)[:, E:]
            self._store(buf.dX[mode], extra, torch.zeros(extra.shape), "dX of the skipped entities")
        # weight gradients per (entity, chunk) item; item -> wavefront item % 2048 -> slab slot
        dz1_w = dz1
        if self.defect == "const_row_leaks_into_dead_columns":
            # no `live` mask on the first-layer operand: a dead lane carries the gradient of the column it read instead (0)
            first = dz1.reshape(32, E, chunks, 32)[:, :, :, :1].expand(32, E, chunks, 32).reshape(32, E, n_col)
            dz1_w = torch.where(live, dz1, first)
        item = lambda t: t.reshape(t.shape[0], E * chunks, 32)  # noqa: E731
        n_items, n_waves = E * chunks, HIST_BLOCKS * WAVES_PER_BLOCK
        wave = torch.arange(n_items) % n_waves
        keep = torch.ones(n_items, dtype=torch.bool)
        if self.defect == "resets_grads_per_item":
            keep = torch.arange(n_items) + n_waves >= n_items      # a wavefront's last item only
        slot = (wave // WAVES_PER_BLOCK if mode == "hist" else wave)[keep]
        for sl, (n, k), dz, a, dzb in zip(buf.slabs[mode], prob.dims, (dz1_w, dz2, dz3), (x, h1, h2), (dz1, dz2, dz3)):
            g = torch.einsum("nib,kib->ink", item(dz[:n]), item(a))      # [items][n][k]
            gb = item(dzb[:n]).sum(dim=2).t()                             # [items][n]
            total = torch.zeros_like(sl)       # summed in registers / LDS first, added to the slot once
            total[:, :, :k].index_add_(0, slot, g[keep])
            total[:, :, k].index_add_(0, slot, gb[keep])
            sl += total

    def reduce(self, prob, buf, mode, scale):
        return [((sl[:, :, :k].sum(dim=0) * scale), (sl[:, :, k].sum(dim=0) * scale))
                for sl, (n, k) in zip(buf.slabs[mode], prob.dims)]
