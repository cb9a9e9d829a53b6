"""Loads tests/golden/*.npz fixtures (written by tests/golden/make_golden.py from the upstream reference)."""
import copy
import json
import os
from collections import defaultdict

import numpy as np
import torch

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


class Golden:
    def __init__(self, name):
        self.name = name
        z = np.load(os.path.join(GOLDEN_DIR, name + ".npz"), allow_pickle=False)
        self.z = z
        self.cfg = json.loads(str(z["cfg_json"]))

    def tensor(self, key):
        return torch.from_numpy(np.array(self.z[key]))

    def group(self, prefix):
        plen = len(prefix) + 1
        return {k[plen:]: self.tensor(k) for k in self.z.files if k.startswith(prefix + "/")}

    @property
    def data(self):
        return self.group("data")

    @property
    def params(self):
        return self.group("param")

    @property
    def grads(self):
        return self.group("grad")

    @property
    def forecaster(self):
        """state dict of the frozen quantile forecaster (quantile policies), or None"""
        f = self.group("forecaster")
        return f or None

    def features(self, t):
        return self.group(f"features/{t}")

    def states(self, t):
        return self.group(f"states/{t}")

    def actions(self, t):
        return self.group(f"actions/{t}")

    def fresh_config(self):
        """Deep copies of the pre-mutation config dicts (Scenario mutates its inputs)."""
        c = copy.deepcopy(self.cfg)
        c["observation_params"] = defaultdict(lambda: None, c["observation_params"])
        return c


# Fixtures on which upstream's env step misplaces orders ACROSS scenarios: a non-zero order on a (store, warehouse) pair whose lead
# time is 0 is added to the element in front of the store's pipeline (environment.py:422-432).  Only the GNN's "j-th connected
# warehouse" action columns (neural_networks.py:1423-1428) produce such orders.  The golden file pins that behaviour for the oracle
# (tests/test_oracle_golden.py); the HIP env step drops such orders, so kernel / engine tests take their expected numbers for
# these cases from the oracle's `zero_lead_orders="drop"` mode.
ZERO_LEAD_CASES = {"f1_many_warehouses_2x10_gnn"}


def tensor_digest(t):
    """dtype, shape and sha256 of a tensor's bytes: equal digests <=> bit-equal tensors (what a fixture stores instead of a
    tensor the test regenerates and compares with torch.equal)."""
    import hashlib
    a = t.detach().cpu().contiguous().numpy() if torch.is_tensor(t) else np.ascontiguousarray(t)
    return f"{a.dtype}{list(a.shape)}:{hashlib.sha256(a.tobytes()).hexdigest()}"


_DATA_ROOT = None


def reference_data_root():
    """A directory holding `data_files/...` as the reference ships them (the Favorita weekly sales, time and sample features,
    per-series cost and lead-time tensors), rebuilt once per process from tests/golden/reference_data.npz.  The settings hold
    paths relative to it, so the real-data cases run with it as the working directory."""
    global _DATA_ROOT
    if _DATA_ROOT is None:
        import tempfile
        z = np.load(os.path.join(GOLDEN_DIR, "reference_data.npz"), allow_pickle=False)
        root = tempfile.mkdtemp(prefix="nic_reference_data_")
        for key in z.files:
            kind, rel = key.split("/", 1)
            if kind == "dtype":
                continue
            path = os.path.join(root, "data_files", rel)
            os.makedirs(os.path.dirname(path), exist_ok=True)
            if kind == "file":
                with open(path, "wb") as f:
                    f.write(z[key].tobytes())
            else:   # a tensor file, stored in the smallest exact dtype
                torch.save(torch.from_numpy(z[key]).to(getattr(torch, str(z["dtype/" + rel]))), path)
        _DATA_ROOT = root
    return _DATA_ROOT


def derived_one_store_file(rows_from=0):
    """The one-store real-data blob the reference does not ship, derived as the fixtures were: every (product, store) series of
    the 21-store weekly sales becomes a one-store sample (series `rows_from`.. of them); returns the path of a temp file."""
    import tempfile
    src = torch.load(os.path.join(reference_data_root(), "data_files/favorita_21_stores/weekly_sales.pt"), map_location="cpu")
    path = os.path.join(tempfile.mkdtemp(), "one.pt")
    torch.save(src.reshape(-1, 1, src.shape[2])[rows_from:].clone(), path)
    return path


def case_names():
    from cases import CASES
    return list(CASES.keys())


def slim_case_names():
    from cases import SLIM_CASES
    return list(SLIM_CASES.keys())


def check_slim_inputs(g, data):
    """A slim fixture holds no inputs: `data` (regenerated from the fixture's seeds) must reproduce the float64 checksums and
    shapes the reference's own tensors had."""
    keys = [k[len("data_checksum/"):] for k in g.z.files if k.startswith("data_checksum/")]
    assert set(keys) == set(data.keys()), (sorted(keys), sorted(data.keys()))
    for k in keys:
        v = data[k]
        assert tuple(v.shape) == tuple(int(x) for x in g.z["data_shape/" + k]), k
        assert float(v.double().sum()) == float(g.z["data_checksum/" + k]), k
        assert float(v.double().abs().sum()) == float(g.z["data_abs_checksum/" + k]), k
