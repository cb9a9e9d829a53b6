"""Generates the fixtures of tests/test_oracle_vs_reference.py and of the real-data cases by RUNNING THE UPSTREAM REFERENCE
(only where its tree is mounted, see reference_harness.py):

    python tests/golden/make_reference_pins.py

  reference_data.npz    the reference's shipped data files (data_files/...) the real-data settings read, in their shapes:
                        tensor files in the smallest dtype that holds them exactly (`dtype/<path>`: the original torch dtype),
                        text files as bytes.  Only what the cases read is kept: the settings take the FIRST rows of a tensor
                        file (rows past KEEP_ROWS are zeroed) and one column of the sample-feature table (the others dropped)
  reference_pins/<pin>.npz   per pinned run: `cfg_json` (the pre-mutation setting / hyperparameter dicts after the overrides,
                        the parameter names, the digests below), `state/<key>` (the reference's policy weights after lazy
                        materialisation), `forecaster/<key>`, `warehouse_upper_bound`, `total`, `reported`, and
                        `grad/<parameter>` where the test compares within a tolerance.  What the test compares bit for bit -
                        the dataset, the final state, the other gradients - is kept as digests (golden_io.tensor_digest).
  reference_configs.json   the reference's YAML files (settings / policies_and_hyperparams) that
                        test_driver_builds_from_reference_config_files reads

The fixtures are DATA (inputs + expected outputs); no reference source text is stored.
"""
import copy
import json
import os
import sys
from collections import defaultdict

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import reference_harness as rh  # noqa: E402
from golden_io import tensor_digest  # noqa: E402
from cases import CASES, apply_overrides  # noqa: E402

PIN_DIR = os.path.join(HERE, "reference_pins")
KEEP_ROWS = {"favorita_21_stores/weekly_sales.pt": 24, "favorita/random_lead_times.pt": 64, "favorita/random_holding_costs.pt": 64,
             "favorita/random_underage_costs.pt": 64}   # (23 products; the derived one-store series 100..139 are products 4-6)
KEEP_COLUMNS = {"favorita/tensors_row_info.csv": ["store_nbr"]}
DATA_FILES = ["favorita_21_stores/weekly_sales.pt", "favorita_21_stores/dates_with_info.csv", "favorita/dates_with_info.csv",
              "favorita/tensors_row_info.csv", "favorita/random_lead_times.pt", "favorita/random_holding_costs.pt",
              "favorita/random_underage_costs.pt"]

# (pin, case name, n, periods, ignore, torch seed, maximize_profit, discrete allocation): the runs test_oracle_vs_reference.py
# compares the oracle with - fresh seeds / sizes beside the golden fixtures, and the variants the YAMLs do not exercise
SYNTHETIC_RUNS = ([(f"fresh/{k}", k, 37, 9, 2, 1234, False, False) for k, v in CASES.items() if not v.get("real")]
                  + [(f"profit/{k}", k, 21, 7, 0, 5, True, False)
                     for k in ("cfg1_one_store_lost_vanilla", "cfg3_one_warehouse_5_vanilla")]
                  + [(f"discrete/{k}", k, 21, 7, 0, 6, False, True)
                     for k in ("cfg1_one_store_lost_vanilla", "cfg2_one_store_backlogged_base_stock",
                               "cfg5_many_warehouses_2x10_vanilla")])
REAL_RUNS = [f"real/{k}" for k, v in CASES.items() if v.get("real")]
REAL_SIZE = dict(n=23, periods=11, ignore=2, period_range="(30, 90)", torch_seed=77, rows_from=100)

DRIVER_PAIRS = [("one_store_lost", "vanilla_one_store"), ("one_store_backlogged", "vanilla_one_store"),
                ("one_store_backlogged", "base_stock"), ("one_store_backlogged", "capped_base_stock"),
                ("one_warehouse_lost_demand", "vanilla_warehouse"), ("many_warehouses_lost_demand", "vanilla_warehouse"),
                ("serial_system", "vanilla_serial"), ("serial_system", "echelon_stock"),
                ("transshipment_backlogged", "vanilla_transshipment"), ("one_warehouse_lost_demand", "gnn")]


def _exact_small(a):
    for dt in (np.int8, np.int16, np.int32, np.float32):
        b = a.astype(dt)
        if np.array_equal(b.astype(a.dtype), a):
            return b
    return a


def data_fixture():
    out = {}
    for rel in DATA_FILES:
        path = os.path.join(rh.REFERENCE_ROOT, "data_files", rel)
        if rel.endswith(".pt"):
            t = torch.load(path, map_location="cpu").clone()
            t[KEEP_ROWS[rel]:] = 0
            out["tensor/" + rel] = _exact_small(t.numpy())
            out["dtype/" + rel] = np.array(str(t.dtype).replace("torch.", ""))
        elif rel in KEEP_COLUMNS:
            import pandas as pd
            text = pd.read_csv(path)[KEEP_COLUMNS[rel]].to_csv(index=False).encode()
            out["file/" + rel] = np.frombuffer(text, dtype=np.uint8)
        else:
            out["file/" + rel] = np.frombuffer(open(path, "rb").read(), dtype=np.uint8)
    return out


def _record(pin, cfg, data, model, total, rep, sim, forecaster=None, exact_grads=False):
    lazy = torch.nn.parameter.UninitializedParameter
    named = [(k, p) for k, p in model.named_parameters() if not isinstance(p, lazy)]
    out = {}
    cfg = dict(cfg, params=[k for k, _ in named], no_grad=[k for k, p in named if p.grad is None],
               data_digest={k: tensor_digest(v) for k, v in data.items()},
               final_digest={k: tensor_digest(sim.observation[k]) for k in ("store_inventories", "warehouse_inventories",
                                                                            "echelon_inventories") if k in sim.observation},
               grad_digest={k: tensor_digest(p.grad) for k, p in named if p.grad is not None} if exact_grads else {})
    out["cfg_json"] = np.array(json.dumps(cfg))
    for k, v in model.state_dict().items():
        if not isinstance(v, lazy):
            out[f"state/{k}"] = v.numpy()
    for k, v in (forecaster or {}).items():
        out[f"forecaster/{k}"] = v.numpy()
    wub = getattr(model, "warehouse_upper_bound", None)
    if torch.is_tensor(wub):
        out["warehouse_upper_bound"] = wub.detach().numpy()
    out["total"] = total.detach().numpy()
    out["reported"] = rep.detach().numpy()
    if not exact_grads:
        for k, p in named:
            if p.grad is not None:
                out[f"grad/{k}"] = p.grad.numpy()
    np.savez_compressed(os.path.join(PIN_DIR, pin.replace("/", "__") + ".npz"), **out)


def synthetic_run(ref, pin, name, n, periods, ignore, torch_seed, maximize_profit, discrete):
    cs, ch = rh.load_reference_configs(CASES[name]["setting"], CASES[name]["policy"])
    cs, ch = apply_overrides(CASES[name], cs, ch)
    cs["problem_params"]["maximize_profit"] = maximize_profit
    cfg = {"cs": copy.deepcopy(cs), "ch": copy.deepcopy(ch), "n": n, "periods": periods, "ignore": ignore, "discrete": discrete}
    obs_r = defaultdict(lambda: None, cs["observation_params"])
    with rh.in_reference_dir():
        sc = ref.Scenario(periods, cs["problem_params"], cs["store_params"], cs["warehouse_params"], cs["echelon_params"], n,
                          obs_r, cs["seeds"])
        data_r = sc.get_data()
        torch.manual_seed(torch_seed)
        model = ref.NeuralNetworkCreator().create_neural_network(sc, ch["nn_params"], device="cpu")
        sim, tr = ref.Simulator(device="cpu"), ref.Trainer(device="cpu")
        o, _ = sim.reset(periods, cs["problem_params"], dict(data_r), obs_r)
        with torch.no_grad():   # materialises the lazy layers
            oo = dict(o)
            oo["internal_data"] = sim._internal_data
            model(oo)
        model.zero_grad()
        total, rep = tr.simulate_batch(ref.PolicyLoss(), sim, model, periods, cs["problem_params"], dict(data_r), obs_r, ignore,
                                       discrete)
        (total / (n * periods * cs["problem_params"]["n_stores"])).backward()
    # (GNN gradients are compared to ~1 ulp, every other policy's bit for bit)
    _record(pin, cfg, data_r, model, total, rep, sim, exact_grads=ch["nn_params"]["name"] != "gnn")


def real_run(ref, pin):
    name = pin.split("/", 1)[1]
    case = CASES[name]
    n, periods, ignore, rng = REAL_SIZE["n"], REAL_SIZE["periods"], REAL_SIZE["ignore"], REAL_SIZE["period_range"]
    cs, ch = rh.load_reference_configs(case["setting"], case["policy"])
    cs, ch = apply_overrides(case, cs, ch)
    cfg = {"cs": copy.deepcopy(cs), "ch": copy.deepcopy(ch), "n": n, "periods": periods, "ignore": ignore,
           "period_range": rng, "one_store_rows_from": REAL_SIZE["rows_from"] if case.get("one_store_from_21") else None}
    if case.get("one_store_from_21"):
        import tempfile
        src = torch.load(os.path.join(rh.REFERENCE_ROOT, "data_files/favorita_21_stores/weekly_sales.pt"), map_location="cpu")
        derived = os.path.join(tempfile.mkdtemp(), "one.pt")
        torch.save(src.reshape(-1, 1, src.shape[2])[REAL_SIZE["rows_from"]:].clone(), derived)
        cs["store_params"]["demand"]["file_location"] = derived
        cfg["cs"]["store_params"]["demand"]["file_location"] = "<derived>"
    obs_r = defaultdict(lambda: None, cs["observation_params"])
    with rh.in_reference_dir():
        sc = ref.Scenario(None, cs["problem_params"], cs["store_params"], cs["warehouse_params"], cs["echelon_params"], n,
                          obs_r, cs["seeds"])
        (ds,) = ref.DatasetCreator().create_datasets(sc, split=True, by_period=True, periods_for_split=[rng])
        torch.manual_seed(REAL_SIZE["torch_seed"])
        model = ref.NeuralNetworkCreator().create_neural_network(sc, ch["nn_params"], device="cpu")
        sim, tr = ref.Simulator(device="cpu"), ref.Trainer(device="cpu")
        total, rep = tr.simulate_batch(ref.PolicyLoss(), sim, model, periods, cs["problem_params"], dict(ds.data), obs_r,
                                       ignore, False)
        if total.requires_grad:
            (total / (n * periods * cs["problem_params"]["n_stores"])).backward()
    fixed = getattr(model, "fixed_nets", None)
    _record(pin, cfg, ds.data, model, total, rep, sim,
            forecaster=fixed["quantile_forecaster"].state_dict() if fixed else None)


def driver_configs():
    import yaml
    cfg = os.path.join(rh.REFERENCE_ROOT, "config_files")
    out = {}
    for setting, policy in DRIVER_PAIRS:
        out[f"settings/{setting}"] = yaml.safe_load(open(f"{cfg}/settings/{setting}.yml"))
        out[f"policies_and_hyperparams/{policy}"] = yaml.safe_load(open(f"{cfg}/policies_and_hyperparams/{policy}.yml"))
    return out


def main():
    ref = rh.load_reference()
    np.savez_compressed(os.path.join(HERE, "reference_data.npz"), **data_fixture())
    with open(os.path.join(HERE, "reference_configs.json"), "w") as f:
        json.dump(driver_configs(), f, indent=1, sort_keys=True)
        f.write("\n")
    os.makedirs(PIN_DIR, exist_ok=True)
    for run in SYNTHETIC_RUNS:
        synthetic_run(ref, *run)
    for pin in REAL_RUNS:
        real_run(ref, pin)
    print(len(SYNTHETIC_RUNS) + len(REAL_RUNS), "runs pinned")


if __name__ == "__main__":
    main()
