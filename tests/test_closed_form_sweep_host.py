"""Host-side surface of the closed-form sweep: the C declaration and its ctypes prototype, the registered operator's fake kernel,
the engine method."""
import os
import re

import torch

from neural_inventory_control_amd import _lib, library  # noqa: F401  (registers the operators)
from neural_inventory_control_amd.closed_form import ClosedFormRollout
from neural_inventory_control_amd.layout import pad_ld

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sweep_entry_point_is_declared_and_bound():
    with open(os.path.join(ROOT, "include", "nic_rollout.h")) as f:
        header = f.read()
    m = re.search(r"int nic_closed_form_sweep\(([^)]*)\);", header)
    assert m, "nic_closed_form_sweep is not declared in include/nic_rollout.h"
    res, args = _lib.PROTOTYPES["nic_closed_form_sweep"]
    assert len(args) == len(m.group(1).split(",")) == 8
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        assert "nic_closed_form_sweep" in f.read()
    assert callable(getattr(ClosedFormRollout, "sweep"))


def test_sweep_operator_has_a_fake_kernel_and_no_autograd_formula():
    from torch._subclasses.fake_tensor import FakeTensorMode
    ld = pad_ld(100)
    with FakeTensorMode():
        for want_grad in (True, False):
            tot, rep, g = torch.ops.nic.sweep_closed_form(torch.empty(7, 2), torch.empty(9, 1, ld), torch.empty(1, 4, ld), 0, 1, 9, 0, 2,
                                                          False, want_grad)
            assert tuple(tot.shape) == (7,) and tuple(rep.shape) == (7,) and tuple(g.shape) == (7, 2)
            assert tot.dtype == rep.dtype == g.dtype == torch.float32
    assert library.sweep_closed_form._setup_context_fn is None and library.sweep_closed_form._backward_fn is None
    assert library.rollout_closed_form._backward_fn is not None   # (the single-candidate operator keeps its formula)
