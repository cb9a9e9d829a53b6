"""Times a whole training step of the reference's underage-cost grid (one_store_lost.yml: 4, 9, 19, 39) x R seeds - I = 4 problem
instances, K = 4 R small policies - two ways, in one process, and writes profiles/small_ensemble_instances_<workload>.json:

  * "inst":  ONE `SmallPolicyEnsemble.train_step` on the list of the I instances' batches (`nic_small_rollout_instances_*`: one
             forward launch, one backward launch, one reduction and one `EnsembleAdam` update for all K models);
  * "seq":   I `train_step`s one after the other, one R-model ensemble with its own `EnsembleAdam` per instance - what the engine
             offered before it took a list of instances;
  each eager and replayed from its captured sequences (`use_graph = True`: "inst_graph", "seq_graph").

    python tools/small_ensemble_instances.py [--workload cfg1] [--scenarios 1024 8192] [--replicas 1 4] [--periods 50] [--reps 15]
                                             [--out-dir profiles]

The scheme of tools/small_ensemble_step.py: device events around each side, every side warmed up, the sides alternated inside every
repetition, the median over the repetitions with the minimum and maximum beside it.  Every cell also checks that both routes, which
saw the same steps, leave equal parameters.  Needs a GPU."""
import argparse
import json
import os
import statistics
import sys
from collections import defaultdict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LR = 1e-3
UNDERAGE = (4.0, 9.0, 19.0, 39.0)


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
    for _ in range(reps):
        for k, fn in sides.items():
            times[k].append(_timed(fn))
    out = {}
    for k, t in times.items():
        out.update({f"{k}_ms": statistics.median(t), f"{k}_min_ms": min(t), f"{k}_max_ms": max(t)})
    out["seq_over_inst"] = out["seq_ms"] / out["inst_ms"]
    out["seq_graph_over_inst_graph"] = out["seq_graph_ms"] / out["inst_graph_ms"]
    return out


def measure(workload, scenarios, replicas, T, reps):
    import torch
    from neural_inventory_control_amd import _lib, workloads
    from neural_inventory_control_amd.data_handling import Scenario
    from neural_inventory_control_amd.ensemble_adam import EnsembleAdam
    from neural_inventory_control_amd.neural_networks import NeuralNetworkCreator
    from neural_inventory_control_amd.policy_layers import materialize_linears
    from neural_inventory_control_amd.small_ensemble import SmallPolicyEnsemble
    dev = "cuda:0"
    setting, policy, _, _, _ = workloads.get(workload)
    pp = setting["problem_params"]
    obs = defaultdict(lambda: None, setting["observation_params"])
    I = len(UNDERAGE)
    out = {"workload": workload, "policy": policy["name"], "periods": T, "reps": reps, "underage_costs": list(UNDERAGE),
           "library_id": _lib.lib().nic_build_id().decode(), "cases": []}
    for n in scenarios:
        datas = []
        for i, u in enumerate(UNDERAGE):   # every cell of the grid: its own demand seed and its underage cost
            seeds = {k: v + 1000 * i if isinstance(v, int) else v for k, v in setting["seeds"].items()}
            sc = Scenario(T, pp, setting["store_params"], setting["warehouse_params"], setting["echelon_params"], n, obs, seeds)
            data = {k: v.to(dev) for k, v in sc.get_data().items()}
            data["underage_costs"] = torch.full_like(data["underage_costs"], u)
            datas.append(data)
        F = datas[0]["initial_inventories"].shape[1] * datas[0]["initial_inventories"].shape[2]

        def models(K):
            ms = []
            for seed in range(K):
                torch.manual_seed(seed)
                m = NeuralNetworkCreator().create_neural_network(sc, policy, device=dev)
                materialize_linears(m.master_linears(), F)
                ms.append(m)
            return ms

        def engine(ms, graph):
            ens = SmallPolicyEnsemble(ms, pp, dev)
            ens.use_graph = graph
            ens.bind_parameters()
            return ens, EnsembleAdam(len(ms), ens.weights.shape[1], dev, lr=LR, param_shapes=ens.param_shapes)
        for R in replicas:
            K = I * R
            inst = {g: engine(models(K), g) for g in (False, True)}
            seq = {g: [engine(models(K)[i * R:(i + 1) * R], g) for i in range(I)] for g in (False, True)}

            def one(g):
                ens, opt = inst[g]
                return lambda: ens.train_step(datas, T, 0, opt, observation_params=obs)

            def loop(g):
                def run():
                    for (ens, opt), data in zip(seq[g], datas):
                        ens.train_step(data, T, 0, opt, observation_params=obs)
                return run
            case = {"n_scenarios": n, "I": I, "R": R, "K": K,
                    **_compare({"inst": one(False), "seq": loop(False), "inst_graph": one(True), "seq_graph": loop(True)}, reps)}
            torch.cuda.synchronize()
            case["parameters_equal"] = bool(all(torch.equal(inst[g][0].weights, torch.cat([ens.weights for ens, _ in seq[g]]))
                                                for g in (False, True)))
            case["kernels"] = dict(inst[False][0].last_kernels)
            out["cases"].append(case)
            print(json.dumps({"workload": workload, **case}), flush=True)
            del inst, seq
            torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workload", default="cfg1")
    ap.add_argument("--scenarios", type=int, nargs="+", default=[1024, 8192])
    ap.add_argument("--replicas", type=int, nargs="+", default=[1, 4])
    ap.add_argument("--periods", type=int, default=50)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    args = ap.parse_args()
    from neural_inventory_control_amd import _lib
    _lib.require_device()
    os.makedirs(args.out_dir, exist_ok=True)
    res = measure(args.workload, args.scenarios, args.replicas, args.periods, args.reps)
    with open(os.path.join(args.out_dir, f"small_ensemble_instances_{args.workload}.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
