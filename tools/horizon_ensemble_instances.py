"""Times a whole training step of K = 16 data_driven policies on I problem instances x R replicas - rollout, gradients and the Adam
update - in one process, and writes profiles/horizon_ensemble_instances_<workload>.json:

  * "list":   `HorizonPolicyEnsemble.train_step` on a LIST of I batches (nic_horizon_rollout_instances_*: one launch pair, the
              model-batched GEMMs and one `EnsembleAdam(K, P)` for all K models);
  * "seq":    I sequential `train_step`s of R-model engines, each on its instance's dict batch with its own `EnsembleAdam(R, P)`:
              what a sweep over settings costs without instances;
  * "single": K x (`FusedRollout.run` + its own fused Adam), every model on its instance's batch.

and, per K in --dict-models, "dict": `train_step` of a K-model engine on ONE dict batch (nic_horizon_rollout_ensemble_*), the path that
must not have become slower.  `--dict-only --tag NAME` times just that and writes ..._<workload>_dict_<NAME>.json: run from a
checkout of the parent commit (the tool uses nothing the parent lacks in that mode) it gives the parent's figures; two such runs
give the parent's own run-to-run spread.  `--parent-runs A.json B.json` (with `--fold-only`: afterwards, without a GPU) folds them into the main file: `dict_slower_than_parent` is
true only where this tree's median exceeds the slower parent run's by more than the two parent runs differ.

    python tools/horizon_ensemble_instances.py [--workloads real_data_driven real_one_store] [--shapes 1x16 4x4 16x1] [--reps 15]

Workloads as tools/horizon_ensemble.py.  Instance i is the workload's batch with its demand and initial pipelines scaled by a
seeded factor and its underage costs by 1 + i (the tables keep their layout).  The scheme of tools/horizon_ensemble_step.py: device
events around each side, every side and shape warmed up, the sides alternated inside every repetition, the median over the
repetitions with the minimum and maximum of each side beside it.  Every cell also checks that "list" and "seq", fed the same
steps, leave equal parameters.  Needs a GPU."""
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
    """sides: {name: callable}; every side warmed up, then alternated inside every repetition"""
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
    return out


def instance_batch(data, i):
    """instance i of a workload's batch (0: the batch itself)"""
    import torch
    if i == 0:
        return data
    gen = torch.Generator().manual_seed(100 + i)
    out = dict(data)
    for k in ("demands", "initial_inventories", "initial_warehouse_inventories"):
        if data.get(k) is not None:
            out[k] = (data[k] * (0.5 + torch.rand(data[k].shape, generator=gen)).to(data[k].device)).contiguous()
    out["underage_costs"] = (data["underage_costs"] * (1.0 + i)).contiguous()
    return out


def measure_dict(workload, model_counts, reps):
    import torch
    import horizon_ensemble as he_tool   # tools/horizon_ensemble.py: the same batches and models
    from neural_inventory_control_amd.ensemble_adam import EnsembleAdam
    cases = []
    for K in model_counts:
        data, obs, n, T, _, ens, _ = he_tool.build(workload, K)
        ens.bind_parameters()
        opt = EnsembleAdam(K, ens.weights.shape[1], "cuda:0", lr=LR, param_shapes=ens.param_shapes)
        case = {"n_scenarios": n, "periods": T, "K": K, **_compare({"dict": lambda: ens.train_step(data, T, 0, opt, obs)}, reps)}
        torch.cuda.synchronize()
        case["kernels"] = dict(ens.last_kernels)
        cases.append(case)
        print(json.dumps({"workload": workload, **case}), flush=True)
        del ens, opt
        torch.cuda.empty_cache()
    return cases


def measure(workload, shapes, reps):
    import torch
    import horizon_ensemble as he_tool
    from neural_inventory_control_amd.ensemble_adam import EnsembleAdam
    from neural_inventory_control_amd.horizon_ensemble import HorizonPolicyEnsemble
    cases = []
    for I, R in shapes:
        K = I * R
        data, obs, n, T, models, ens, _ = he_tool.build(workload, K)
        batches = [instance_batch(data, i) for i in range(I)]
        ens.bind_parameters()
        P = ens.weights.shape[1]
        opt = EnsembleAdam(K, P, "cuda:0", lr=LR, param_shapes=ens.param_shapes)
        _, _, _, _, models_s, _, _ = he_tool.build(workload, K)
        seq = []
        for i in range(I):
            e = HorizonPolicyEnsemble(models_s[i * R:(i + 1) * R], ens.problem_params, "cuda:0")
            e.bind_parameters()
            seq.append((e, EnsembleAdam(R, P, "cuda:0", lr=LR, param_shapes=e.param_shapes)))
        _, _, _, _, _, _, singles = he_tool.build(workload, K)
        opts_d = [torch.optim.Adam(eng.model.parameters(), lr=LR, fused=True) for eng in singles]

        def listed():
            ens.train_step(batches, T, 0, opt, obs)

        def sequential():
            for i, (e, o) in enumerate(seq):
                e.train_step(batches[i], T, 0, o, obs)

        def single():
            for m, (eng, o) in enumerate(zip(singles, opts_d)):
                eng.run(batches[m // R], T, 0, train=True, observation_params=obs)
                o.step()
        case = {"n_scenarios": n, "periods": T, "K": K, "I": I, "R": R,
                **_compare({"list": listed, "seq": sequential, "single": single}, reps)}
        torch.cuda.synchronize()
        case["seq_over_list"] = case["seq_ms"] / case["list_ms"]
        case["single_over_list"] = case["single_ms"] / case["list_ms"]
        case["list_slower_than_seq"] = bool(case["list_ms"] > case["seq_ms"])
        case["list_seq_parameters_equal"] = bool(torch.equal(ens.weights, torch.cat([e.weights for e, _ in seq])))
        case["kernels"] = {**ens.last_kernels, **opt.last_kernels}
        cases.append(case)
        print(json.dumps({"workload": workload, **case}), flush=True)
        del ens, opt, seq, singles, opts_d, models, models_s, batches
        torch.cuda.empty_cache()
    return cases


def fold_parent(cases, parent_runs):
    """dict cases of this tree against two runs of the parent's: the bar is the parent's own run-to-run difference"""
    runs = []
    for path in parent_runs:
        with open(path) as f:
            runs.append({c["K"]: c for c in json.load(f)["dict_cases"]})
    out = []
    for c in cases:
        a, b = (r[c["K"]]["dict_ms"] for r in runs)
        spread = abs(a - b)
        out.append({"K": c["K"], "dict_ms": c["dict_ms"], "parent_a_ms": a, "parent_b_ms": b, "parent_spread_ms": spread,
                    "dict_over_parent": c["dict_ms"] / (0.5 * (a + b)), "dict_slower_than_parent": bool(c["dict_ms"] > max(a, b) + spread)})
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workloads", nargs="+", default=["real_data_driven", "real_one_store"])
    ap.add_argument("--shapes", nargs="+", default=["1x16", "4x4", "16x1"], help="IxR")
    ap.add_argument("--dict-models", type=int, nargs="+", default=[1, 4, 16])
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--dict-only", action="store_true")
    ap.add_argument("--tag", default="run")
    ap.add_argument("--parent-runs", nargs=2, metavar="JSON", help="two --dict-only files of the parent commit, with {workload} in the name")
    ap.add_argument("--fold-only", action="store_true", help="no measurement: fold --parent-runs into the main files of --out-dir")
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    args = ap.parse_args()
    if args.reps < 15:
        ap.error("at least 15 repetitions")
    if args.fold_only:
        for name in args.workloads:
            path = os.path.join(args.out_dir, f"horizon_ensemble_instances_{name}.json")
            with open(path) as f:
                res = json.load(f)
            res["dict_vs_parent"] = fold_parent(res["dict_cases"], [p.format(workload=name) for p in args.parent_runs])
            with open(path, "w") as f:
                json.dump(res, f, indent=1)
                f.write("\n")
        return
    from neural_inventory_control_amd import _lib
    _lib.require_device()
    os.makedirs(args.out_dir, exist_ok=True)
    shapes = [tuple(int(v) for v in s.split("x")) for s in args.shapes]
    for name in args.workloads:
        res = {"workload": name, "reps": args.reps, "library_id": _lib.lib().nic_build_id().decode()}
        res["dict_cases"] = measure_dict(name, args.dict_models, args.reps)
        if args.dict_only:
            path = os.path.join(args.out_dir, f"horizon_ensemble_instances_{name}_dict_{args.tag}.json")
        else:
            res["cases"] = measure(name, shapes, args.reps)
            if args.parent_runs:
                res["dict_vs_parent"] = fold_parent(res["dict_cases"], [p.format(workload=name) for p in args.parent_runs])
            path = os.path.join(args.out_dir, f"horizon_ensemble_instances_{name}.json")
        with open(path, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
