"""Times a WHOLE training step of K = 16 data_driven policies on one real-data batch when some of them have stopped training (the
active-model mask, `HorizonPolicyEnsemble.skip_inactive`) - in one process - and writes profiles/horizon_active_step_<workload>.json:

  * "b":   `HorizonPolicyEnsemble.train_step` at K = 16, `skip_inactive = False`, no mask set: the launch sequence of the commit
           before the mask reached this engine's launches;
  * "b2":  (b) again on a second engine: two runs of the same code in this process;
  * "c":   `skip_inactive = True` with an all-ones mask: the `_active` entry points, all 16 models run (and the totals' NaN masking);
  * "d8", "d4", "d1": `skip_inactive = True` with 8 / 4 / 1 of the 16 models active (the first ones: grid rows 8.. / 4.. / 1.. return
           at entry);
  * "k8", "k4", "k1": engines of K = 8 / 4 / 1 models with no mask: what a sweep rebuilt without the stopped models would pay - the
           yardstick of (d).  (16 active: (c) against (b).)
  * "glue16": the torch glue of a K = 16 step alone, on (b)'s buffers - the `W1obs.copy_`, the copy of the observation rows into
           the other K - 1 models' `X` and `slabs[i].zero_()`, which follow no mask; "glue8", "glue4", "glue1": the same for the (k)
           engines (K = 1 has no replica to copy to).
           `dN_glue_excess_ms` = glue16 - glueN: the part of d - k the glue explains.

    python tools/horizon_active_step.py [--workloads real_one_store real_data_driven] [--reps 20] [--out-dir profiles] [--merge-parent FILE ...]
    python tools/horizon_active_step.py --unmasked-only --out FILE      # sides b ("a" in FILE), k8, k4, k1 alone
    python tools/horizon_active_step.py --merge-only --merge-parent FILE ...   # fold parent runs into profiles already written
    python tools/horizon_active_step.py --trace-side d1 --workloads real_one_store --steps 10   # one side alone, for a kernel trace

`--unmasked-only` uses nothing the commit before lacks, so the same file run in a checkout of THAT commit measures (a), the
parent's step, and the parent's smaller-K engines (e); `--merge-parent` folds such files into the profile: every parent run's median
[min, max] per side, the envelope of the parent's samples and, for (b) and (c), whether the median lies inside it and the
difference to the parent's median; (d) over the parent's (k) per active count.  `--trace-side` runs warm-up + `--steps` steps of one
side and nothing else: under `rocprofv3 --kernel-trace --stats` (a run of its own) it gives the kernel time of that side, which
splits d - k into the empty workgroups (kernel time) and the rest (glue, launches); `--kernel-stats d1=FILE k1=FILE ...` with
`--merge-only` folds the totals of such `*_kernel_stats.csv` files into the profile.

Workloads as tools/horizon_ensemble.py: `real_one_store` (8,192 series x 95 weeks: 512 workgroups per model, one model fills the
device) and `real_data_driven` (72 products x 21 stores x 3 warehouses x T = 95: 5 workgroups per model).  Device events around each
side, every side warmed up, the sides alternated inside every repetition in an order that rotates from one repetition to the next,
the median over the repetitions with each side's minimum and maximum beside it.  Every run also checks that (b), (b2) and (c) leave
equal parameters, that (d)'s returned totals are NaN exactly on the stopped models, that their weights rows did not move and that
the active rows are (b)'s.  Needs a GPU."""
import argparse
import csv
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
LR, K_FULL = 1e-3, 16
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


def _engine(workload, K):
    """(batch, observation params, scenarios, periods, a bound engine of K models, its optimizer)"""
    import horizon_ensemble as he_tool   # tools/horizon_ensemble.py: the same batches and models
    from neural_inventory_control_amd.ensemble_adam import EnsembleAdam
    data, obs, n, T, _, ens, singles = he_tool.build(workload, K)
    del singles
    ens.bind_parameters()
    return data, obs, n, T, ens, EnsembleAdam(K, ens.weights.shape[1], "cuda:0", lr=LR, param_shapes=ens.param_shapes)


def _glue(ens):
    """the torch glue of a dict-batch step on the engine's buffers (after a first step sized them): what follows no mask"""
    from neural_inventory_control_amd.ensemble_step import layer_slices
    K, FD, Fo = ens.n_models, ens.F_dyn, ens.F - ens.F_dyn
    o, n, k, _ = layer_slices(ens.dims)[0]
    X = ens.X   # [K][F][T][ld]: one batch for all K models = one instance with K replicas

    def fn():
        if K > 1:
            X[1:, FD:].copy_(X[:1, FD:].expand(K - 1, Fo, X.shape[2], X.shape[3]))
        ens.W1obs[:, :, :Fo].copy_(ens.weights[:, o:o + n * k].view(K, n, k)[:, :, FD:])
        for slab in ens.slabs:
            slab.zero_()
    return fn


def _side_setup(name, ens):
    if name in ("a", "b", "b2") or name.startswith("k"):
        return
    ens.skip_inactive = True
    count = K_FULL if name == "c" else int(name[1:])
    ens.set_active([1] * count + [0] * (K_FULL - count))


def measure(workload, reps, unmasked_only):
    import torch
    from neural_inventory_control_amd import _lib
    out = {"workload": workload, "K": K_FULL, "reps": reps, "library_id": _lib.lib().nic_build_id().decode()}
    names = ["a"] if unmasked_only else ["b", "b2", "c"] + [f"d{c}" for c in ACTIVE_COUNTS]
    bound, data, obs, T = {}, None, None, None
    for name in names + [f"k{c}" for c in ACTIVE_COUNTS]:
        K = int(name[1:]) if name.startswith("k") else K_FULL
        data, obs, n, T, ens, opt = _engine(workload, K)
        _side_setup(name, ens)
        bound[name] = (ens, opt)
        out.update(n_scenarios=n, periods=T)
    start = {name: ens.weights.clone() for name, (ens, _) in bound.items()}
    last = {}

    def step(name):
        ens, opt = bound[name]

        def fn():
            last[name] = ens.train_step(data, T, 0, opt, obs)
        return fn
    sides = {name: step(name) for name in bound}
    for fn in sides.values():   # (a first step sizes every engine's buffers: the glue sides need them)
        fn()
    if not unmasked_only:
        sides["glue16"] = _glue(bound["b"][0])
        for c in ACTIVE_COUNTS:
            sides[f"glue{c}"] = _glue(bound[f"k{c}"][0])
    out.update(_compare(sides, reps))
    torch.cuda.synchronize()
    if not unmasked_only:
        same = lambda x, y: bool(torch.equal(bound[x][0].weights, bound[y][0].weights))  # noqa: E731
        out["b_b2_parameters_equal"], out["b_c_parameters_equal"] = same("b", "b2"), same("b", "c")
        out["c_minus_b_ms"] = out["c_ms"] - out["b_ms"]
        out["b_spread_ms"] = max(out["b_max_ms"], out["b2_max_ms"]) - min(out["b_min_ms"], out["b2_min_ms"])
        for count in ACTIVE_COUNTS:
            ens, _ = bound[f"d{count}"]
            total = last[f"d{count}"][0]
            out[f"d{count}_totals_nan_on_stopped_only"] = torch.isnan(total).tolist() == [False] * count + [True] * (K_FULL - count)
            out[f"d{count}_stopped_rows_unmoved"] = bool(torch.equal(ens.weights[count:], start[f"d{count}"][count:]))
            out[f"d{count}_active_rows_equal_b"] = bool(torch.equal(ens.weights[:count], bound["b"][0].weights[:count]))
            out[f"d{count}_over_k{count}"] = out[f"d{count}_ms"] / out[f"k{count}_ms"]
            out[f"d{count}_over_b"] = out[f"d{count}_ms"] / out["b_ms"]
            out[f"d{count}_minus_k{count}_ms"] = out[f"d{count}_ms"] - out[f"k{count}_ms"]
            out[f"d{count}_glue_excess_ms"] = out["glue16_ms"] - out[f"glue{count}_ms"]
        out["kernels"] = {name: {**bound[name][0].last_kernels, **bound[name][1].last_kernels} for name in ("b", "c", "d1")}
        out["model_gemms_ran"] = bool(bound["b"][0]._models_ok)
    print(json.dumps(out), flush=True)
    return out


def trace_side(workload, name, steps):
    """warm-up + `steps` steps of one side, nothing else on the device: the run a kernel trace is taken of"""
    import torch
    K = int(name[1:]) if name.startswith("k") else K_FULL
    data, obs, _, T, ens, opt = _engine(workload, K)
    _side_setup(name, ens)
    for _ in range(3 + steps):
        ens.train_step(data, T, 0, opt, obs)
    torch.cuda.synchronize()
    print(json.dumps({"workload": workload, "side": name, "steps": 3 + steps}))


def merge_parent(profile, parent_files):
    """the parent's runs (`--unmasked-only` in a checkout of the commit before) into the profile of the same workload"""
    runs = []
    for path in parent_files:
        with open(path) as f:
            runs += [res for res in json.load(f) if res["workload"] == profile["workload"]]
    if not runs:
        return
    profile["parent_library_ids"] = sorted({r["library_id"] for r in runs})
    for side in ("a",) + tuple(f"k{c}" for c in ACTIVE_COUNTS):
        profile[f"parent_{side}_runs_ms"] = [[r[f"{side}_ms"], r[f"{side}_min_ms"], r[f"{side}_max_ms"]] for r in runs]
    medians = [r["a_ms"] for r in runs]
    lo, hi = min(r["a_min_ms"] for r in runs), max(r["a_max_ms"] for r in runs)
    profile["parent_a_ms"] = statistics.median(medians)
    profile["parent_medians_differ_ms"] = max(medians) - min(medians)
    profile["parent_samples_envelope_ms"] = [lo, hi]
    for side in ("b", "c"):
        profile[f"{side}_inside_parent_envelope"] = bool(lo <= profile[f"{side}_ms"] <= hi)
        profile[f"{side}_minus_parent_a_ms"] = profile[f"{side}_ms"] - profile["parent_a_ms"]
    for count in ACTIVE_COUNTS:
        e = statistics.median(r[f"k{count}_ms"] for r in runs)
        profile[f"parent_e{count}_ms"] = e
        profile[f"d{count}_over_parent_e{count}"] = profile[f"d{count}_ms"] / e
    profile["d16_over_parent_e16"] = profile["c_ms"] / profile["parent_a_ms"]


def merge_kernel_stats(profile, stats, steps):
    """`side=FILE` pairs of rocprofv3 `*_kernel_stats.csv` files of `--trace-side` runs: the kernel time per step of each side"""
    for item in stats:
        side, path = item.split("=", 1)
        with open(path) as f:
            rows = list(csv.DictReader(f))
        total_ns = sum(float(r["TotalDurationNs"]) for r in rows)
        ours = [r for r in rows if "at::native" not in r["Name"] and "rocclr" not in r["Name"]]   # (the library's kernels)
        copies = [r for r in rows if "direct_copy_kernel" in r["Name"]]
        profile[f"{side}_kernel_ms_per_step"] = total_ns / 1e6 / steps   # (all kernels, the run's set-up fills and copies included)
        profile[f"{side}_library_kernel_ms_per_step"] = sum(float(r["TotalDurationNs"]) for r in ours) / 1e6 / steps
        profile[f"{side}_torch_copy_kernels"] = [sum(int(r["Calls"]) for r in copies), sum(float(r["TotalDurationNs"]) for r in copies) / 1e6]
        profile[f"{side}_kernels_ms_per_step"] = {r["Name"][:60]: float(r["TotalDurationNs"]) / 1e6 / steps
                                                  for r in sorted(rows, key=lambda r: -float(r["TotalDurationNs"]))[:8]}
    for count in ACTIVE_COUNTS:
        d, k = profile.get(f"d{count}_kernel_ms_per_step"), profile.get(f"k{count}_kernel_ms_per_step")
        if d is not None and k is not None:
            profile[f"d{count}_kernel_excess_ms"] = d - k   # (all kernels; the K = 16 engine's larger set-up is in it)
            # the empty workgroups of the stopped models: the library's kernels alone
            profile[f"d{count}_library_kernel_excess_ms"] = (profile[f"d{count}_library_kernel_ms_per_step"]
                                                             - profile[f"k{count}_library_kernel_ms_per_step"])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workloads", nargs="+", default=["real_one_store", "real_data_driven"])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--unmasked-only", action="store_true", help="sides a, k8, k4, k1 alone: runs in a checkout without the feature too")
    ap.add_argument("--out", help="with --unmasked-only: the JSON file to write")
    ap.add_argument("--merge-parent", nargs="*", default=[], help="files --unmasked-only wrote in a checkout of the commit before")
    ap.add_argument("--merge-only", action="store_true", help="measure nothing: fold --merge-parent / --kernel-stats into the profiles in --out-dir")
    ap.add_argument("--kernel-stats", nargs="*", default=[], help="side=FILE: rocprofv3 kernel stats of --trace-side runs (one workload)")
    ap.add_argument("--trace-side", help="run one side alone (b, c, d8, d4, d1, k8, k4, k1) for a kernel trace")
    ap.add_argument("--steps", type=int, default=10, help="with --trace-side: timed steps after 3 warm-up steps (all are traced)")
    args = ap.parse_args()
    if args.merge_only:
        for name in args.workloads:
            path = os.path.join(args.out_dir, f"horizon_active_step_{name}.json")
            with open(path) as f:
                res = json.load(f)
            merge_parent(res, args.merge_parent)
            merge_kernel_stats(res, args.kernel_stats, 3 + args.steps)
            with open(path, "w") as f:
                json.dump(res, f, indent=1)
                f.write("\n")
        return
    from neural_inventory_control_amd import _lib
    _lib.require_device()
    if args.trace_side:
        trace_side(args.workloads[0], args.trace_side, args.steps)
        return
    results = [measure(name, args.reps, args.unmasked_only) for name in args.workloads]
    if args.unmasked_only:
        with open(args.out or "horizon_active_step_unmasked.json", "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")
        return
    os.makedirs(args.out_dir, exist_ok=True)
    for res in results:
        merge_parent(res, args.merge_parent)
        with open(os.path.join(args.out_dir, f"horizon_active_step_{res['workload']}.json"), "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
