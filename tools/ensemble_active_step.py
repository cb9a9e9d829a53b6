"""Times a WHOLE training step of K = 16 small policies when some of them have stopped training (the active-model mask of the
`_active` entry points, `EnsembleStep.set_active`) - in one process, eager and replayed - and writes
profiles/ensemble_active_step_<scenarios>.json:

  * "b":  `SmallPolicyEnsemble.train_step` at K = 16 with no mask set: the launch sequence of the commit before the mask;
  * "b2": (b) again on a second engine: two runs of the same code in this process;
  * "c":  the same step after `set_active` with every model active: the `_active` entry points, all 16 models run;
  * "d8", "d4", "d1": 8 / 4 / 1 of the 16 models active (the first ones: grid rows 8.. / 4.. / 1.. return at entry);
  * "k8", "k4", "k1": engines of K = 8 / 4 / 1 models with no mask: what a sweep that had been rebuilt without the stopped models
          would pay - the yardstick of (d).

    python tools/ensemble_active_step.py [--scenarios 1024 32768] [--reps 30] [--out-dir profiles] [--merge-parent FILE ...]
    python tools/ensemble_active_step.py --unmasked-only --out FILE      # sides b ("a" in FILE), k8, k4, k1 alone
    python tools/ensemble_active_step.py --merge-only --merge-parent FILE ...   # fold parent runs into profiles already written

`--unmasked-only` uses nothing the commit before the mask lacks, so the same file run in a checkout of THAT commit measures (a),
the parent's step, and the parent's smaller-K engines; `--merge-parent` folds such files into the profile: every parent run's
median [min, max] per cell, the spread of the parent's own runs (`parent_medians_differ_ms`, the envelope of their samples) and,
for (b) and (c), whether the median lies inside that envelope and how far it is above the slower parent run.  Nothing is asked
of (d): it is reported next to (k) as measured.

One-store lost demand (cfg1's setting and policy), T = 50.  Device events around each side, every side warmed up (a replayed side's
first call of a shape is eager, the second captures), the sides alternated inside every repetition in an order that rotates from
one repetition to the next, the median over the repetitions with each side's minimum and maximum beside it.  Every cell also checks
that (b), (b2) and (c) leave equal parameters, that (d)'s returned totals are NaN exactly on the stopped models and that their
weights rows did not move.  Needs a GPU."""
import argparse
import json
import os
import statistics
import sys
from collections import defaultdict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LR, K_FULL, T_STEP = 1e-3, 16, 50
ACTIVE_COUNTS = (8, 4, 1)


def _timed(fn):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def _compare(sides, reps, warmup=3):
    for _ in range(warmup):
        for fn in sides.values():
            fn()
    times = {k: [] for k in sides}
    names = list(sides)
    for r in range(reps):   # (the order rotates: what a side's place in the round costs it is spread over all sides)
        for k in names[r % len(names):] + names[:r % len(names)]:
            times[k].append(_timed(sides[k]))
    out = {}
    for k, t in times.items():
        out.update({f"{k}_ms": statistics.median(t), f"{k}_min_ms": min(t), f"{k}_max_ms": max(t)})
    return out


def _batch(n):
    """cfg1's batch of n scenarios, the keywords of `train_step` and a builder of bound engines of K models with their optimizer"""
    import torch
    from neural_inventory_control_amd import workloads
    from neural_inventory_control_amd.data_handling import Scenario
    from neural_inventory_control_amd.neural_networks import NeuralNetworkCreator
    from neural_inventory_control_amd.policy_layers import materialize_linears
    from neural_inventory_control_amd.small_ensemble import SmallPolicyEnsemble
    dev = "cuda:0"
    setting, policy, _, _, _ = workloads.get("cfg1")
    pp = setting["problem_params"]
    obs = defaultdict(lambda: None, setting["observation_params"])
    sc = Scenario(T_STEP, pp, setting["store_params"], setting["warehouse_params"], setting["echelon_params"], n, obs, dict(setting["seeds"]),
                  sampler="hip", device=dev)
    data = {k: v.to(dev) for k, v in sc.get_data().items()}
    F = data["initial_inventories"].shape[1] * data["initial_inventories"].shape[2]

    def engine(K, use_graph):
        models = []
        for seed in range(K):
            torch.manual_seed(seed)
            m = NeuralNetworkCreator().create_neural_network(sc, policy, device=dev)
            materialize_linears(m.master_linears(), F)
            models.append(m)
        ens = SmallPolicyEnsemble(models, pp, dev)
        ens.use_graph = use_graph
        ens.bind_parameters()
        return ens, ens.make_optimizer(LR, max_grad_norm=None)
    return data, dict(observation_params=obs, demand_soa=sc.demands_soa), engine


def measure(n, reps, unmasked_only):
    import torch
    from neural_inventory_control_amd import _lib
    data, kw, engine = _batch(n)
    out = {"n_scenarios": n, "periods": T_STEP, "K": K_FULL, "reps": reps, "library_id": _lib.lib().nic_build_id().decode(), "cases": []}
    for graph in (False, True):
        bound = {"a" if unmasked_only else "b": engine(K_FULL, graph)}
        if not unmasked_only:
            bound["b2"] = engine(K_FULL, graph)
            for name, count in [("c", K_FULL)] + [(f"d{c}", c) for c in ACTIVE_COUNTS]:
                bound[name] = engine(K_FULL, graph)
                bound[name][0].set_active([1] * count + [0] * (K_FULL - count))
        for count in ACTIVE_COUNTS:
            bound[f"k{count}"] = engine(count, graph)
        start = {name: ens.weights.clone() for name, (ens, _) in bound.items()}
        last = {}

        def step(name):
            ens, opt = bound[name]

            def fn():
                last[name] = ens.train_step(data, T_STEP, 0, opt, **kw)
            return fn
        case = {"replayed": graph, **_compare({name: step(name) for name in bound}, reps)}
        torch.cuda.synchronize()
        if not unmasked_only:
            same = lambda x, y: bool(torch.equal(bound[x][0].weights, bound[y][0].weights))  # noqa: E731
            case["b_b2_parameters_equal"], case["b_c_parameters_equal"] = same("b", "b2"), same("b", "c")
            for count in ACTIVE_COUNTS:
                ens, opt = bound[f"d{count}"]
                total = last[f"d{count}"][0]
                case[f"d{count}_totals_nan_on_stopped_only"] = torch.isnan(total).tolist() == [False] * count + [True] * (K_FULL - count)
                case[f"d{count}_stopped_rows_unmoved"] = bool(torch.equal(ens.weights[count:], start[f"d{count}"][count:]))
                case[f"d{count}_active_rows_equal_b"] = bool(torch.equal(ens.weights[:count], bound["b"][0].weights[:count]))
                case[f"d{count}_over_k{count}"] = case[f"d{count}_ms"] / case[f"k{count}_ms"]
                case[f"d{count}_over_b"] = case[f"d{count}_ms"] / case["b_ms"]
            case["b_spread_ms"] = max(case["b_max_ms"], case["b2_max_ms"]) - min(case["b_min_ms"], case["b2_min_ms"])
            case["kernels"] = {"b": {**bound["b"][0].last_kernels, **bound["b"][1].last_kernels},
                               "c": {**bound["c"][0].last_kernels, **bound["c"][1].last_kernels}}
        if graph:
            case["captures"] = {name: len(ens._graphs) for name, (ens, _) in bound.items()}
        out["cases"].append(case)
        print(json.dumps({"n_scenarios": n, **case}), flush=True)
        del bound, start, last
        torch.cuda.empty_cache()
    return out


def merge_parent(profile, parent_files):
    """the parent's runs (`--unmasked-only` in a checkout of the commit before) into the profile's cells of the same batch"""
    runs = []
    for path in parent_files:
        with open(path) as f:
            for res in json.load(f):
                if res["n_scenarios"] == profile["n_scenarios"]:
                    runs.append(res)
    if not runs:
        return
    profile["parent_library_ids"] = sorted({r["library_id"] for r in runs})
    for case in profile["cases"]:
        cells = [c for r in runs for c in r["cases"] if c["replayed"] == case["replayed"]]
        if not cells:
            continue
        for side in ("a",) + tuple(f"k{c}" for c in ACTIVE_COUNTS):
            case[f"parent_{side}_runs_ms"] = [[c[f"{side}_ms"], c[f"{side}_min_ms"], c[f"{side}_max_ms"]] for c in cells]
        medians = [c["a_ms"] for c in cells]
        lo, hi = min(c["a_min_ms"] for c in cells), max(c["a_max_ms"] for c in cells)
        case["parent_medians_differ_ms"] = max(medians) - min(medians)
        case["parent_samples_envelope_ms"] = [lo, hi]
        for side in ("b", "c"):
            case[f"{side}_inside_parent_envelope"] = bool(lo <= case[f"{side}_ms"] <= hi)
            case[f"{side}_over_slower_parent_run_ms"] = case[f"{side}_ms"] - max(medians)
        for count in ACTIVE_COUNTS:
            case[f"d{count}_over_parent_k{count}"] = case[f"d{count}_ms"] / statistics.median(c[f"k{count}_ms"] for c in cells)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scenarios", type=int, nargs="+", default=[1024, 32768])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--unmasked-only", action="store_true", help="sides a, k8, k4, k1 alone: runs in a checkout without the mask too")
    ap.add_argument("--out", help="with --unmasked-only: the JSON file to write")
    ap.add_argument("--merge-parent", nargs="*", default=[], help="files --unmasked-only wrote in a checkout of the commit before")
    ap.add_argument("--merge-only", action="store_true", help="measure nothing: fold --merge-parent into the profiles already in --out-dir")
    args = ap.parse_args()
    if args.merge_only:
        for n in args.scenarios:
            path = os.path.join(args.out_dir, f"ensemble_active_step_{n}.json")
            with open(path) as f:
                res = json.load(f)
            merge_parent(res, args.merge_parent)
            with open(path, "w") as f:
                json.dump(res, f, indent=1)
                f.write("\n")
        return
    from neural_inventory_control_amd import _lib
    _lib.require_device()
    results = [measure(n, args.reps, args.unmasked_only) for n in args.scenarios]
    if args.unmasked_only:
        with open(args.out or "ensemble_active_step_unmasked.json", "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")
        return
    os.makedirs(args.out_dir, exist_ok=True)
    for res in results:
        merge_parent(res, args.merge_parent)
        with open(os.path.join(args.out_dir, f"ensemble_active_step_{res['n_scenarios']}.json"), "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
