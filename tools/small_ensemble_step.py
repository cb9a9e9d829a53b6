"""Times a WHOLE training step of K small policies on one batch - rollout, gradients AND the Adam update - four ways, in one process,
and writes profiles/small_ensemble_step_<workload>.json:

  * "a": `SmallPolicyEnsemble.train_step` with bound parameters and an `EnsembleAdam`, eager (six launches);
  * "b": the same, replayed from its captured sequence (`use_graph = True`);
  * "c": the whole step without them: `SmallPolicyEnsemble.run` (packs the weights, assigns the gradients) + ONE
         `torch.optim.Adam(fused=True)` with K parameter groups;
  * "d": K x (`FusedRollout.run` + its own fused Adam), the single-model route once per model.

    python tools/small_ensemble_step.py [--workloads cfg1 cfg2 cfg4] [--scenarios 1024 8192 32768] [--models 1 4 16] [--periods 50]
                                        [--reps 15] [--out-dir profiles]

The scheme of tools/small_ensemble.py: device events around each side, every side warmed up, the sides alternated inside every
repetition, the median over the repetitions with the minimum and maximum of the comparison sides beside it.  A cell MISSES a
condition only outside the comparison side's own min-max spread: `b_slower_than_c` (every cell), `b_slower_than_d` (K = 1).  Every
cell also checks that (a) and (b), which saw the same steps, leave equal parameters.  Needs a GPU."""
import argparse
import json
import os
import statistics
import sys
from collections import defaultdict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LR = 1e-3


def _timed(fn):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def _compare(sides, reps, warmup=3):
    """sides: {name: callable}.  (warm-up of "b": the first call of a shape is eager, the second captures)"""
    for _ in range(warmup):
        for fn in sides.values():
            fn()
    times = {k: [] for k in sides}
    for _ in range(reps):
        for k, fn in sides.items():
            times[k].append(_timed(fn))
    out = {}
    for k, t in times.items():
        out.update({f"{k}_ms": statistics.median(t), f"{k}_min_ms": min(t), f"{k}_max_ms": max(t)})
    for k in ("c", "d"):
        out[f"{k}_spread_ms"] = out[f"{k}_max_ms"] - out[f"{k}_min_ms"]
        out[f"{k}_over_b"] = out[f"{k}_ms"] / out["b_ms"]
    out["b_slower_than_c"] = bool(out["b_ms"] > out["c_ms"] + out["c_spread_ms"])
    out["b_slower_than_d"] = bool(out["b_ms"] > out["d_ms"] + out["d_spread_ms"])
    return out


def measure(workload, scenarios, model_counts, T, reps):
    import torch
    from neural_inventory_control_amd import _lib, workloads
    from neural_inventory_control_amd.data_handling import Scenario
    from neural_inventory_control_amd.ensemble_adam import EnsembleAdam
    from neural_inventory_control_amd.neural_networks import NeuralNetworkCreator
    from neural_inventory_control_amd.policy_layers import materialize_linears
    from neural_inventory_control_amd.rollout import FusedRollout
    from neural_inventory_control_amd.small_ensemble import SmallPolicyEnsemble
    dev = "cuda:0"
    setting, policy, _, _, _ = workloads.get(workload)
    pp = setting["problem_params"]
    obs = defaultdict(lambda: None, setting["observation_params"])
    out = {"workload": workload, "policy": policy["name"], "periods": T, "reps": reps, "library_id": _lib.lib().nic_build_id().decode(),
           "cases": []}
    for n in scenarios:
        sc = Scenario(T, pp, setting["store_params"], setting["warehouse_params"], setting["echelon_params"], n, obs, dict(setting["seeds"]),
                      sampler="hip", device=dev)
        data = {k: v.to(dev) for k, v in sc.get_data().items()}
        F = data["initial_inventories"].shape[1] * data["initial_inventories"].shape[2]
        if policy["name"] != "vanilla_one_store":
            F += sum(v.shape[1] * v.shape[2] for k, v in data.items() if k in ("initial_warehouse_inventories", "initial_echelon_inventories"))
        kw = dict(observation_params=obs, demand_soa=sc.demands_soa)

        def models(K):
            ms = []
            for seed in range(K):
                torch.manual_seed(seed)
                m = NeuralNetworkCreator().create_neural_network(sc, policy, device=dev)
                materialize_linears(m.master_linears(), F)
                ms.append(m)
            return ms
        for K in model_counts:
            bound = {}
            for side, graph in (("a", False), ("b", True)):
                ens = SmallPolicyEnsemble(models(K), pp, dev)
                ens.use_graph = graph
                ens.bind_parameters()
                opt = EnsembleAdam(K, ens.weights.shape[1], dev, lr=LR, param_shapes=ens.param_shapes)
                bound[side] = (ens, opt)
            ens_c = SmallPolicyEnsemble(models(K), pp, dev)
            opt_c = torch.optim.Adam([{"params": list(m.parameters())} for m in ens_c.models], lr=LR, fused=True)
            singles = [FusedRollout(m, pp, dev) for m in models(K)]
            opts_d = [torch.optim.Adam(eng.model.parameters(), lr=LR, fused=True) for eng in singles]

            def step(side):
                ens, opt = bound[side]
                return lambda: ens.train_step(data, T, 0, opt, **kw)

            def c():
                ens_c.run(data, T, 0, train=True, **kw)
                opt_c.step()

            def d():
                for eng, opt in zip(singles, opts_d):
                    eng.run(data, T, 0, train=True, **kw)
                    opt.step()
            case = {"n_scenarios": n, "K": K, **_compare({"a": step("a"), "b": step("b"), "c": c, "d": d}, reps)}
            torch.cuda.synchronize()
            (ens_a, opt_a), (ens_b, opt_b) = bound["a"], bound["b"]
            case["a_b_parameters_equal"] = bool(torch.equal(ens_a.weights, ens_b.weights) and torch.equal(opt_a.state, opt_b.state))
            case["b_captures"] = len(ens_b._graphs)
            case["kernels"] = {**ens_a.last_kernels, **opt_a.last_kernels}
            out["cases"].append(case)
            print(json.dumps({"workload": workload, **case}), flush=True)
            del bound, ens_a, ens_b, opt_a, opt_b, ens_c, opt_c, singles, opts_d
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
        with open(os.path.join(args.out_dir, f"small_ensemble_step_{name}.json"), "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
