"""`bench.py --dump-outputs`: the arrays of the last timed step go to DIR/<name>.npy within a fixed byte budget; above it a
larger array is replaced by a seeded sample of its entries, the same in every run."""
import numpy as np
import torch

import bench


def test_dump_outputs_writes_every_array_within_the_budget(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 1 << 16)
    model = torch.nn.Linear(100, 200)
    model(torch.ones(3, 100)).sum().backward()
    outs = bench.step_outputs(model, total_cost=12.5)
    assert outs["total_cost"].dtype == torch.float64 and outs["param.weight"].dtype == torch.float32
    for run in ("a", "b"):
        bench.dump_outputs(str(tmp_path / run), outs)
    files = {p.name: np.load(p) for p in (tmp_path / "a").glob("*.npy")}
    assert set(files) == {"total_cost.npy", "param.weight.npy", "param.bias.npy", "grad.weight.npy", "grad.bias.npy"}
    assert sum(a.nbytes for a in files.values()) <= 1 << 16
    assert float(files["total_cost.npy"]) == 12.5
    np.testing.assert_array_equal(files["param.bias.npy"], model.bias.detach().numpy())   # small enough: whole
    w = files["param.weight.npy"]
    assert w.ndim == 1 and 0 < w.size < model.weight.numel() and np.isin(w, model.weight.detach().numpy()).all()
    for name, a in files.items():   # the same sample in every run
        np.testing.assert_array_equal(a, np.load(tmp_path / "b" / name))
