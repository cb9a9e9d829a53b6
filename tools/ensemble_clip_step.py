"""Times a WHOLE training step of K policies with every model's gradient norm clipped - rollout, gradients, clipping AND the Adam
update - in one process, and writes profiles/ensemble_clip_step_<workload>.json:

  * "a": `train_step` with bound parameters and an `EnsembleAdam(max_grad_norm=1.0)`: the clipped optimizer launches
         (`nic_ensemble_adam_prepare_clipped` / `_update_clipped`), still two;
  * "b": the same step with an `EnsembleAdam` that was never given a max norm: the launch sequence of the commit before clipping;
  * "b2": (b) again on a second engine: two runs of the same code, what a difference between sides has to exceed;
  * "c": clipped training without the clipped launches: `run(train=True)` (packs the weights, assigns the gradients) + K x
         `torch.nn.utils.clip_grad_norm_(model.parameters(), 1.0)` + ONE `torch.optim.Adam(fused=True)` with K parameter groups;
  * "ar", "br" (small policies only): (a) and (b) replayed from their captured sequences (`use_graph = True`).

    python tools/ensemble_clip_step.py [--workloads cfg1 real_data_driven] [--models 1 4 16] [--reps 30] [--out-dir profiles]

Workloads: `cfg1` - K `vanilla_one_store` policies (`SmallPolicyEnsemble`) on 1,024 scenarios x T = 50, as
tools/small_ensemble_step.py; `real_data_driven` - K `data_driven` policies (`HorizonPolicyEnsemble`) on the 72-product real-data
batch, as tools/horizon_ensemble_step.py.  The scheme of those tools: device events around each side, every side warmed up, the
sides alternated inside every repetition (here in an order that rotates from one repetition to the next), the median over the repetitions with the minimum and maximum of each side beside it.  No
ratio is asked of (a); the one condition is on (b), whose launches are those of the commit before: `b_slower_than_parent` is set
when its median lies above the maximum that commit's own profile recorded for the same cell (side "a" of
profiles/small_ensemble_step_cfg1.json / profiles/horizon_ensemble_step_real_data_driven.json - another session, so the two runs
of (b) beside it say what one session's spread is).  Every cell also checks that the max norm of 1.0 did clip, that (b) and (b2)
leave equal parameters and, for the small policies, that replayed and eager steps do.  Needs a GPU."""
import argparse
import json
import os
import statistics
import sys
from collections import defaultdict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
LR, MAX_NORM = 1e-3, 1.0
PARENT = {"cfg1": "small_ensemble_step_cfg1.json", "real_data_driven": "horizon_ensemble_step_real_data_driven.json"}


def _timed(fn):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def _compare(sides, reps, warmup=3):
    """sides: {name: callable}.  (warm-up of a replayed side: the first call of a shape is eager, the second captures)"""
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
    for k in sides:
        if k != "a":
            out[f"{k}_over_a"] = out[f"{k}_ms"] / out["a_ms"]
    return out


def _parent_cell(workload, n, K):
    """the commit before's recorded step (side "a" of its profile) for this cell, or None"""
    try:
        with open(os.path.join(ROOT, "profiles", PARENT[workload])) as f:
            prof = json.load(f)
    except OSError:
        return None
    for c in prof["cases"]:
        if (c["n_scenarios"], c["K"]) == (n, K):
            return {"parent_ms": c["a_ms"], "parent_min_ms": c["a_min_ms"], "parent_max_ms": c["a_max_ms"], "parent_library_id": prof["library_id"]}
    return None


def _small(K, T=50, n=1024):
    """cfg1: the batch, its size, T, the keywords of `run` / `train_step` and a builder of fresh unbound engines of K models"""
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
    sc = Scenario(T, pp, setting["store_params"], setting["warehouse_params"], setting["echelon_params"], n, obs, dict(setting["seeds"]),
                  sampler="hip", device=dev)
    data = {k: v.to(dev) for k, v in sc.get_data().items()}
    F = data["initial_inventories"].shape[1] * data["initial_inventories"].shape[2]

    def engine(use_graph=False):
        models = []
        for seed in range(K):
            torch.manual_seed(seed)
            m = NeuralNetworkCreator().create_neural_network(sc, policy, device=dev)
            materialize_linears(m.master_linears(), F)
            models.append(m)
        ens = SmallPolicyEnsemble(models, pp, dev)
        ens.use_graph = use_graph
        return ens
    return data, n, T, dict(observation_params=obs, demand_soa=sc.demands_soa), engine


def _horizon(K):
    """the same for the 72-product real-data batch"""
    import horizon_ensemble as he_tool   # tools/horizon_ensemble.py: the same batch and models
    data, obs, n, T, _, _, _ = he_tool.build("real_data_driven", 1)
    return data, n, T, dict(observation_params=obs), lambda use_graph=False: he_tool.build("real_data_driven", K)[5]


def measure(workload, model_counts, reps):
    import torch
    from neural_inventory_control_amd import _lib
    out = {"workload": workload, "max_norm": MAX_NORM, "reps": reps, "library_id": _lib.lib().nic_build_id().decode(), "cases": []}
    for K in model_counts:
        data, n, T, kw, engine = _small(K) if workload == "cfg1" else _horizon(K)
        out.update(n_scenarios=n, periods=T)
        bound = {}
        for side, clip, graph in (("a", MAX_NORM, False), ("b", None, False), ("b2", None, False), ("ar", MAX_NORM, True), ("br", None, True)):
            if graph and workload != "cfg1":
                continue
            ens = engine(graph)
            ens.bind_parameters()
            bound[side] = (ens, ens.make_optimizer(LR, max_grad_norm=clip))
        ens_c = engine()
        opt_c = torch.optim.Adam([{"params": list(m.parameters())} for m in ens_c.models], lr=LR, fused=True)

        def step(side):
            ens, opt = bound[side]
            return lambda: ens.train_step(data, T, 0, opt, **kw)

        def c():
            ens_c.run(data, T, 0, train=True, **kw)
            for m in ens_c.models:
                torch.nn.utils.clip_grad_norm_(m.parameters(), MAX_NORM)
            opt_c.step()
        case = {"n_scenarios": n, "K": K, **_compare({**{s: step(s) for s in bound}, "c": c}, reps)}
        torch.cuda.synchronize()
        same = lambda x, y: bool(torch.equal(bound[x][0].weights, bound[y][0].weights) and torch.equal(bound[x][1].state, bound[y][1].state))  # noqa: E731
        case["b_b2_parameters_equal"] = same("b", "b2")
        if "ar" in bound:
            case["a_ar_parameters_equal"], case["b_br_parameters_equal"] = same("a", "ar"), same("b", "br")
            case["ar_captures"], case["br_captures"] = len(bound["ar"][0]._graphs), len(bound["br"][0]._graphs)
        opt_a = bound["a"][1]
        case["a_clip_scales_min_max"] = [float(opt_a.clip_scales.min()), float(opt_a.clip_scales.max())]
        case["a_grad_norms_min_max"] = [float(opt_a.grad_norms.min()), float(opt_a.grad_norms.max())]
        case["a_clipped_every_model"] = bool((opt_a.clip_scales < 1).all())
        case["b_spread_ms"] = max(case["b_max_ms"], case["b2_max_ms"]) - min(case["b_min_ms"], case["b2_min_ms"])
        parent = _parent_cell(workload, n, K)
        if parent is not None:
            case.update(parent)
            case["b_slower_than_parent"] = bool(case["b_ms"] > parent["parent_max_ms"])
        case["kernels"] = {"a": dict(opt_a.last_kernels), "b": dict(bound["b"][1].last_kernels)}
        out["cases"].append(case)
        print(json.dumps({"workload": workload, **case}), flush=True)
        del bound, ens_c, opt_c, opt_a
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workloads", nargs="+", default=["cfg1", "real_data_driven"], choices=sorted(PARENT))
    ap.add_argument("--models", type=int, nargs="+", default=[1, 4, 16])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    args = ap.parse_args()
    from neural_inventory_control_amd import _lib
    _lib.require_device()
    os.makedirs(args.out_dir, exist_ok=True)
    for name in args.workloads:
        res = measure(name, args.models, args.reps)
        with open(os.path.join(args.out_dir, f"ensemble_clip_step_{name}.json"), "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
