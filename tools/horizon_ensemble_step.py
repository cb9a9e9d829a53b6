"""Times a WHOLE training step of K data_driven policies on one real-data batch - rollout, gradients AND the Adam update - in one
process, and writes profiles/horizon_ensemble_step_<workload>.json:

  * "a": `HorizonPolicyEnsemble.train_step` with bound parameters and an `EnsembleAdam`: the launch pair, the model-batched GEMMs
         (one launch for all K models each) and the optimizer's two launches;
  * "e": the same step with `model_gemms = False` (the per-model loop of single-model GEMM calls): what the batching alone buys;
  * "c": the whole step without any of it: `HorizonPolicyEnsemble.run` with `model_gemms = False` (packs the weights, K x the GEMMs,
         assigns the gradients) + ONE `torch.optim.Adam(fused=True)` with K parameter groups - the parent commit's step, but for
         six reads of `nic_last_kernel` a step that its loop did not make;
  * "d": K x (`FusedRollout.run` + its own fused Adam), the single-model route once per model.

    python tools/horizon_ensemble_step.py [--workloads real_data_driven real_one_store] [--models 1 4 16] [--reps 15] [--out-dir profiles]

Workloads as tools/horizon_ensemble.py: `real_data_driven` (72 products x 21 stores x 3 warehouses x T = 95) and `real_one_store`
(8,192 series x 95 weeks).  The scheme of tools/small_ensemble_step.py: device events around each side, every side warmed up, the
sides alternated inside every repetition, the median over the repetitions with the minimum and maximum of each side beside it.  A
cell MISSES only when (a) is slower than (c) outside (c)'s own min-max spread: `a_slower_than_c`.  Every cell also checks that (a) and
(e), two engines fed the same steps with `model_gemms` on and off, leave equal parameters and optimizer state.  Needs a GPU."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
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
    """sides: {name: callable}"""
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
    for k in ("e", "c", "d"):
        out[f"{k}_over_a"] = out[f"{k}_ms"] / out["a_ms"]
    out["c_spread_ms"] = out["c_max_ms"] - out["c_min_ms"]
    out["a_slower_than_c"] = bool(out["a_ms"] > out["c_ms"] + out["c_spread_ms"])
    return out


def measure(workload, model_counts, reps):
    import torch
    import horizon_ensemble as he_tool   # tools/horizon_ensemble.py: the same batches and models
    from neural_inventory_control_amd import _lib
    from neural_inventory_control_amd.ensemble_adam import EnsembleAdam
    out = {"workload": workload, "reps": reps, "library_id": _lib.lib().nic_build_id().decode(), "cases": []}
    for K in model_counts:
        bound = {}
        for side, gemms in (("a", True), ("e", False)):
            data, obs, n, T, _, ens, _ = he_tool.build(workload, K)
            ens.model_gemms = gemms
            ens.bind_parameters()
            bound[side] = (ens, EnsembleAdam(K, ens.weights.shape[1], "cuda:0", lr=LR, param_shapes=ens.param_shapes))
        _, _, _, _, models_c, ens_c, _ = he_tool.build(workload, K)
        ens_c.model_gemms = False
        opt_c = torch.optim.Adam([{"params": list(m.parameters())} for m in models_c], lr=LR, fused=True)
        _, _, _, _, _, _, singles = he_tool.build(workload, K)
        opts_d = [torch.optim.Adam(eng.model.parameters(), lr=LR, fused=True) for eng in singles]
        out.update(n_scenarios=n, periods=T)

        def step(side):
            ens, opt = bound[side]
            return lambda: ens.train_step(data, T, 0, opt, obs)

        def c():
            ens_c.run(data, T, 0, train=True, observation_params=obs)
            opt_c.step()

        def d():
            for eng, opt in zip(singles, opts_d):
                eng.run(data, T, 0, train=True, observation_params=obs)
                opt.step()
        case = {"n_scenarios": n, "K": K, **_compare({"a": step("a"), "e": step("e"), "c": c, "d": d}, reps)}
        torch.cuda.synchronize()
        (ens_a, opt_a), (ens_e, opt_e) = bound["a"], bound["e"]
        case["a_e_parameters_equal"] = bool(torch.equal(ens_a.weights, ens_e.weights) and torch.equal(opt_a.state, opt_e.state)
                                            and torch.equal(opt_a.exp_avg, opt_e.exp_avg) and torch.equal(opt_a.exp_avg_sq, opt_e.exp_avg_sq))
        case["a_model_gemms_ran"] = bool(ens_a._models_ok)
        case["kernels"] = {**ens_a.last_kernels, **opt_a.last_kernels}
        out["cases"].append(case)
        print(json.dumps({"workload": workload, **case}), flush=True)
        del bound, ens_a, ens_e, opt_a, opt_e, ens_c, opt_c, models_c, singles, opts_d
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workloads", nargs="+", default=["real_data_driven", "real_one_store"])
    ap.add_argument("--models", type=int, nargs="+", default=[1, 4, 16])
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    args = ap.parse_args()
    from neural_inventory_control_amd import _lib
    _lib.require_device()
    os.makedirs(args.out_dir, exist_ok=True)
    for name in args.workloads:
        res = measure(name, args.models, args.reps)
        with open(os.path.join(args.out_dir, f"horizon_ensemble_step_{name}.json"), "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
