"""Times a step of K small policies on one batch two ways, in one process, and writes profiles/small_ensemble_<workload>.json:

  * "ensemble": `SmallPolicyEnsemble.run` - one forward launch, one backward launch and one reduction for all K models;
  * "loop":     K `FusedRollout.run` steps of the unchanged single-model route, one engine per model.

    python tools/small_ensemble.py [--workloads cfg1 cfg2 cfg4] [--scenarios 1024 8192 32768] [--models 1 4 16] [--periods 50]
                                   [--reps 15] [--out-dir profiles]

Training (forward + backward + reduce) and evaluation (forward + cost sums).  Device events around each side, both sides warmed
up, the two sides alternated inside every repetition; the median over the repetitions is reported with the minimum and maximum of
each side beside it.  A cell counts as slower than the loop only if its median exceeds the loop's median by more than the loop's
own min-max spread (`slower_than_loop`).  Needs a GPU."""
import argparse
import json
import os
import statistics
import sys
from collections import defaultdict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _timed(fn):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def _compare(ensemble, loop, reps, warmup=3):
    for _ in range(warmup):
        ensemble()
        loop()
    te, tl = [], []
    for _ in range(reps):
        te.append(_timed(ensemble))
        tl.append(_timed(loop))
    me, ml = statistics.median(te), statistics.median(tl)
    spread = max(tl) - min(tl)
    return {"ensemble_ms": me, "loop_ms": ml, "ensemble_min_ms": min(te), "ensemble_max_ms": max(te), "loop_min_ms": min(tl),
            "loop_max_ms": max(tl), "loop_spread_ms": spread, "loop_over_ensemble": ml / me, "slower_than_loop": bool(me > ml + spread)}


def measure(workload, scenarios, model_counts, T, reps):
    import torch
    from neural_inventory_control_amd import _lib, workloads
    from neural_inventory_control_amd.data_handling import Scenario
    from neural_inventory_control_amd.neural_networks import NeuralNetworkCreator
    from neural_inventory_control_amd.policy_layers import materialize_linears
    from neural_inventory_control_amd.rollout import FusedRollout
    from neural_inventory_control_amd.small_ensemble import SmallPolicyEnsemble
    dev = "cuda:0"
    setting, policy, _, _, _ = workloads.get(workload)
    obs = defaultdict(lambda: None, setting["observation_params"])
    out = {"workload": workload, "policy": policy["name"], "periods": T, "reps": reps, "library_id": _lib.lib().nic_build_id().decode(),
           "cases": []}
    for n in scenarios:
        sc = Scenario(T, setting["problem_params"], setting["store_params"], setting["warehouse_params"], setting["echelon_params"], n,
                      obs, dict(setting["seeds"]), sampler="hip", device=dev)
        data = {k: v.to(dev) for k, v in sc.get_data().items()}
        F = data["initial_inventories"].shape[1] * data["initial_inventories"].shape[2]
        if policy["name"] != "vanilla_one_store":
            F += sum(v.shape[1] * v.shape[2] for k, v in data.items() if k in ("initial_warehouse_inventories", "initial_echelon_inventories"))
        kw = dict(observation_params=obs, demand_soa=sc.demands_soa)
        for K in model_counts:
            models = []
            for seed in range(K):
                torch.manual_seed(seed)
                m = NeuralNetworkCreator().create_neural_network(sc, policy, device=dev)
                materialize_linears(m.master_linears(), F)
                models.append(m)
            ens = SmallPolicyEnsemble(models, setting["problem_params"], dev)
            singles = [FusedRollout(m, setting["problem_params"], dev) for m in models]
            for train in (True, False):
                def ensemble():
                    ens.run(data, T, 0, train=train, **kw)

                def loop():
                    for eng in singles:
                        eng.run(data, T, 0, train=train, **kw)
                case = {"n_scenarios": n, "K": K, "train": train, **_compare(ensemble, loop, reps)}
                tot, _ = ens.run(data, T, 0, train=train, **kw)
                case["kernels"] = dict(ens.last_kernels)
                case["totals_equal"] = all(bool(torch.equal(tot[i], eng.run(data, T, 0, train=train, **kw)[0])) for i, eng in enumerate(singles))
                out["cases"].append(case)
                print(json.dumps({"workload": workload, **case}), flush=True)
            del ens, singles, models
            torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workloads", nargs="+", default=["cfg1", "cfg2", "cfg4"])
    ap.add_argument("--scenarios", type=int, nargs="+", default=[1024, 8192, 32768])
    ap.add_argument("--models", type=int, nargs="+", default=[1, 4, 16])
    ap.add_argument("--periods", type=int, default=50)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    args = ap.parse_args()
    from neural_inventory_control_amd import _lib
    _lib.require_device()
    os.makedirs(args.out_dir, exist_ok=True)
    for name in args.workloads:
        res = measure(name, args.scenarios, args.models, args.periods, args.reps)
        with open(os.path.join(args.out_dir, f"small_ensemble_{name}.json"), "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
