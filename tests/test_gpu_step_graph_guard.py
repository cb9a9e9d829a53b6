"""The stream-hazard self-test that `Trainer.use_step_graph = "auto"` relies on (Trainer._stream_hazard_is_reported) runs once per
device and process.  Its first call may come from an evaluation epoch, which runs under torch.no_grad(): the probe must give the
same answer there as under grad mode, or every later training step of the process is refused its capture."""
import pytest
import torch

from neural_inventory_control_amd.trainer import Trainer

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def test_stream_hazard_probe_does_not_depend_on_the_callers_grad_mode():
    saved = dict(Trainer._hazard_guard)
    try:
        Trainer._hazard_guard.clear()
        with_grad = Trainer._stream_hazard_is_reported(DEV)
        Trainer._hazard_guard.clear()
        with torch.no_grad():
            under_no_grad = Trainer._stream_hazard_is_reported(DEV)
        assert with_grad is True   # (this stack reports the hazard: the step-graph tests depend on it)
        assert under_no_grad is True
    finally:
        Trainer._hazard_guard.clear()
        Trainer._hazard_guard.update(saved)
