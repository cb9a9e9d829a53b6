"""Exact emulation of the bf16 GEMMs (csrc/linear_bf16.hip) and the error bounds their tests use.  Works on any device.

Emulation: operands rounded to bf16 by torch (`tensor.to(torch.bfloat16)`: round to nearest even), contracted in float64.  A
bf16 x bf16 product is exact in FP32 (8 + 8 mantissa bits), so the only thing a correct kernel adds is the rounding of its FP32
additions: for a sum of n terms in ANY order and ANY grouping (MFMA trees, flush segments, slab slots, the reduction over slots)

    |C - C_ref| <= n * 2^-24 * sum |a| |b|       (n - 1 additions, each off by at most 2^-24 of a partial sum <= sum |a||b|)

plus one FP32 rounding each for the bias add (2 * 2^-24 * |z + bias| allows for it and the rounding of z it is added to), the
ELU (its polynomial / __expf approximation: 3e-7 * (1 + |z|), measured for the FP32 kernels whose epilogue this is; ELU is
1-Lipschitz, so the error of z passes through unamplified) and ELU' (y + 1 and the product: 2 * 2^-24 * |z| ELU').  A slab that is
not zero to begin with adds one rounding of (base + partial sum) per += that carries at least one term - at most n of them,
whatever the slot split (adding an empty partial sum is exact): n * 2^-24 * max over the slots of |base|.

Power: the bound grows like n^2 (n * sum over n terms) while one lost or doubled 32-scenario tile stays the size of 32 terms, so
beyond ~7,000 terms a dense contraction cannot show such a tile any more - and a weight gradient that crosses a flush segment
has more than 8,192 terms per output by construction.  `tile_scan_stride` / `tile_mask` give passes over the same launch that
keep every m-th tile only (same-sign operands), in each of which a single tile stands >= 20 x above the bound again.

Every function returns (reference, bound) pairs as float64 tensors; `worst` is the largest |got - ref| / bound."""
import torch

U = 2.0 ** -24
ELU_ABS = 3e-7      # the FP32 kernels' ELU approximation, absolute + relative part
TINY = 1e-30        # keeps 0 / 0 out of the ratio where reference and bound are both exactly 0


def bf(t):
    """bf16 rounding of an FP32 tensor (torch's cast: round to nearest even), as float64"""
    return t.to(torch.bfloat16).double()


def elu(z):
    return torch.where(z > 0, z, torch.expm1(torch.clamp(z, max=0)))


def elu_grad_from_out(h):
    return torch.where(h > 0, torch.ones_like(h), h + 1)


def worst(got, ref, tol):
    """largest |got - ref| / tol (float64 on the tensors' device; 0.0 for empty tensors)"""
    if ref.numel() == 0:
        return 0.0
    return float(((got.double() - ref).abs() / tol).max())


def within(got, ref, tol, what):
    w = worst(got, ref, tol)
    assert w <= 1.0, f"{what}: worst error / bound = {w:.3g}"
    return w


def forward(W, X, bias=None, act_elu=True):
    """Y = act(bf16(W)[N][K] bf16(X)[K][n] + bias): (Y, bound)"""
    a, b = bf(W), bf(X)
    K = a.shape[1]
    z = a @ b
    S = a.abs() @ b.abs()
    tol = K * U * S + TINY
    if bias is not None:
        z = z + bias.double()[:, None]
        tol = tol + 2 * U * z.abs()
    if act_elu:
        tol = tol + ELU_ABS * (1 + z.abs())
        z = elu(z)
    return z, tol


def dgrad(Wt, dY, H=None, prev=None):
    """dX = (bf16(Wt)[K][N] bf16(dY)[N][n]) * ELU'(H) (+ prev); H None: no activation.  (dX, bound)"""
    a, b = bf(Wt), bf(dY)
    N = a.shape[1]
    z = a @ b
    S = a.abs() @ b.abs()
    d = elu_grad_from_out(H.double()) if H is not None else torch.ones_like(z)
    ref = z * d + (prev.double() if prev is not None else 0)
    tol = (N * U * S + 2 * U * z.abs()) * d + 2 * U * ref.abs() + TINY
    return ref, tol


def wgrad(dY, X, repeats=1, base_w=None, base_b=None):
    """dW = repeats * bf16(dY)[N][n] bf16(X)[K][n]^T and db = repeats * sum_b dY (FP32 operands): (dW, bound, db, bound).
    base_w / base_b: the largest |slab content| over the slots that the sums were added to, see the module docstring."""
    a, b = bf(dY), bf(X)
    terms = repeats * a.shape[1]
    ref = repeats * (a @ b.t())
    S = repeats * (a.abs() @ b.abs().t())
    dyd = dY.double()
    ref_b, S_b = repeats * dyd.sum(1), repeats * dyd.abs().sum(1)
    tol, tol_b = terms * U * S + TINY, terms * U * S_b + TINY
    if base_w is not None:
        tol = tol + terms * U * base_w.double().abs()
    if base_b is not None:
        tol_b = tol_b + terms * U * base_b.double().abs()
    return ref, tol, ref_b, tol_b


def wgrad_periods(dYh, Xh, base_w=None, base_b=None):
    """`wgrad` over histories dYh [T][N][n], Xh [T][K][n]: one contraction over (period, scenario)"""
    T, N, n = dYh.shape
    return wgrad(dYh.permute(1, 0, 2).reshape(N, T * n), Xh.permute(1, 0, 2).reshape(Xh.shape[1], T * n), 1, base_w, base_b)


TILE = 32   # scenarios per LDS tile of the weight-gradient kernel (BK in csrc/linear_bf16.hip)


def tile_scan_stride(terms, power=20.0):
    """m (a power of two) such that in a pass that keeps every m-th 32-scenario tile of a contraction of `terms` terms, operands
    all of one sign and of even magnitude, one tile is >= `power` x the bound: the tile is TILE * m / terms of that pass's
    sum |a||b|, the bound terms * 2^-24 of it."""
    m = 1
    while TILE * m < power * terms * terms * U:
        m *= 2
    return m


def tile_mask(T, n, ncols, m, r, device):
    """[T][ncols] bool: the columns < n whose (period, 32-scenario tile) index is r modulo m"""
    col = torch.arange(ncols, device=device)[None, :]
    tile = torch.arange(T, device=device)[:, None] * ((n + TILE - 1) // TILE) + col // TILE
    return (tile % m == r) & (col < n)
