"""The fused gather-MLP kernels (csrc/mlp3.hip) element-wise against float64 on the layouts GnnRollout hands them: the case table
and the checker of tests/mlp3_checks.py through the HIP backend (tests/test_mlp3_checks_host.py shows on the CPU that the checker
notices each class of kernel error), and the argument checks of the launchers."""
import pytest
import torch

import mlp3_checks as mc
from neural_inventory_control_amd import _lib, ops

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", mc.CASES, ids=[c.id for c in mc.CASES])
def test_mlp3_against_float64(case):
    backend = mc.HipMlp3()
    figures = mc.check_case(case, backend)     # (asserts that the variants expected_kernels() names are the ones that ran;
    #                                             test_the_table_reaches_every_dispatch_cell: they cover every launcher cell)
    print(case.id, " ".join(mc.expected_kernels(case)), "worst err / bound:",
          "  ".join(f"{k} {v:.2f}" for k, v in figures.items()))


def _launchable(n_rows=7, E=3, B=40):
    """A small valid launch: descriptor arguments and buffers (nothing is launched here)."""
    dev, ld = "cuda", mc.pad32(B)
    dims = [(32, n_rows), (32, 32), (32, 32)]
    packed = torch.zeros(sum(n * k + n for n, k in dims), device=dev)
    packed_t = torch.zeros(n_rows * 32 + 32 + 2 * (32 * 32 + 32), device=dev)
    z = lambda r: torch.zeros(r, E, ld, device=dev)  # noqa: E731
    slabs = [torch.zeros(ops.mlp3_bwd_hist_slots(), n, (k + 1 + 3) // 4 * 4, device=dev) for n, k in dims]
    return dict(segs=[ops.Mlp3Segment(z(n_rows))], packed=packed, packed_t=packed_t, E=E, B=B, ld=ld, z=z, slabs=slabs)


def _desc(a, segs=None, ld=None, **kw):
    return ops.mlp3_desc(segs or a["segs"], a["packed"], a["E"], a["B"], ld or a["ld"], 32, 1, 0, a["packed_t"], **kw)


def test_mlp3_argument_checks_refuse_on_the_host():
    """Each of these is refused by `validate` or a launcher before any launch (only arguments the host rejects are passed)."""
    a = _launchable()
    z, E, ld = a["z"], a["E"], a["ld"]
    with pytest.raises(_lib.NicError, match=r"K \(97\)"):                      # K = 97
        ops.mlp3_fwd(_desc(a, segs=[ops.Mlp3Segment(z(97))]), z(32))
    five = _desc(a)
    five.n_segs = 5                                                     # (the descriptor holds four: only the count says five)
    with pytest.raises(_lib.NicError, match="segments"):
        ops.mlp3_fwd(five, z(32))
    with pytest.raises(_lib.NicError, match="ent_row_stride"):
        ops.mlp3_fwd(_desc(a, ent_row_stride=E * ld - 32), z(32))
    with pytest.raises(_lib.NicError, match="native"):
        ops.mlp3_fwd(_desc(a, hist_native=True), z(32), z(7), z(32), z(32))
    with pytest.raises(_lib.NicError, match="native"):
        ops.mlp3_bwd_hist(_desc(a, hist_native=True), z(32), z(32), z(7), z(32), z(32), z(7), a["slabs"])
    with pytest.raises(_lib.NicError, match="aligned"):                # H1 one float past a 16-byte boundary
        ops.mlp3_bwd_hist(_desc(a), z(32), z(32), z(7), torch.zeros(32 * E * ld + 4, device="cuda")[1:], z(32), z(7), a["slabs"])
    with pytest.raises(_lib.NicError, match="multiple of 32"):
        ops.mlp3_fwd(_desc(a, ld=40), torch.zeros(32, E, 40, device="cuda"))
    torch.cuda.synchronize()
