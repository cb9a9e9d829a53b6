"""Times the closed-form sweep (`ClosedFormRollout.sweep`: K candidate level vectors in one launch) against what it replaces, K
sequential single-candidate rollouts (`ClosedFormRollout.run`, the unchanged kernel), for base_stock, capped_base_stock and
echelon_stock, with and without level gradients, and writes profiles/closed_form_sweep_<policy>.json.

    python tools/closed_form_sweep.py [--scenarios 32768] [--periods 100] [--candidates 16 64] [--reps 30] [--out-dir profiles]

Two pairs of figures per (K, gradients): "api" = the engine's methods as a user calls them (per call: state packing, launch, the
sum over wavefronts), "kernel" = the C-ABI launches alone (one nic_closed_form_sweep against K nic_closed_form_rollout_sums).
Device events around each side, both sides warmed up, the two sides alternated inside every repetition (neighbours on a shared
host disturb both alike); the median over the repetitions is reported, the minimum beside it.  Needs a GPU.
--lib PATH times another build of the library (e.g. one compiled with -DNIC_CF_SWEEP_TRY_KC=4 to compare group sizes)."""
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


def _compare(sweep, loop, reps, warmup=3):
    for _ in range(warmup):
        sweep()
        loop()
    ts, tl = [], []
    for _ in range(reps):
        ts.append(_timed(sweep))
        tl.append(_timed(loop))
    ms, ml = statistics.median(ts), statistics.median(tl)
    return {"sweep_ms": ms, "loop_ms": ml, "sweep_min_ms": min(ts), "loop_min_ms": min(tl), "loop_over_sweep": ml / ms}


def measure(policy_name, n, T, candidates, reps):
    import torch
    from neural_inventory_control_amd import _lib, closed_form, workloads
    from neural_inventory_control_amd.closed_form import ClosedFormRollout
    from neural_inventory_control_amd.data_handling import Scenario
    from neural_inventory_control_amd.neural_networks import NeuralNetworkCreator
    dev = "cuda:0"
    setting, policy, _, _, _ = workloads.get("echelon_stock" if policy_name == "echelon_stock" else "base_stock")
    if policy_name == "capped_base_stock":
        policy = workloads._closed_form("capped_base_stock", 2)
    obs = defaultdict(lambda: None, setting["observation_params"])
    sc = Scenario(T, setting["problem_params"], setting["store_params"], setting["warehouse_params"], setting["echelon_params"], n,
                  obs, dict(setting["seeds"]), sampler="hip", device=dev)
    data = {k: v.to(dev) for k, v in sc.get_data().items()}
    torch.manual_seed(5)
    model = NeuralNetworkCreator().create_neural_network(sc, policy, device=dev)
    eng = ClosedFormRollout(model, setting["problem_params"], dev)
    with torch.no_grad():
        base = model.closed_form_levels().detach().clone()
    if policy_name == "capped_base_stock":
        base = base * torch.tensor([2.2, 0.7], device=dev)
    kw = dict(observation_params=setting["observation_params"], demand_soa=sc.demands_soa)
    lib = _lib.lib()
    out = {"policy": policy_name, "n_scenarios": n, "periods": T, "reps": reps, "library_id": lib.nic_build_id().decode(), "cases": []}
    for K in candidates:
        levels = (base[None, :] * torch.linspace(0.5, 2.0, K, device=dev)[:, None]).contiguous()
        rows = [levels[k].clone() for k in range(K)]
        for want_grad in (True, False):
            def api_sweep():
                eng.sweep(levels, data, T, 0, want_grad=want_grad, **kw)

            def api_loop():
                for row in rows:
                    model.closed_form_levels = lambda row=row: row.requires_grad_(want_grad)
                    with torch.set_grad_enabled(want_grad):
                        eng.run(data, T, 0, train=want_grad, **kw)
            case = {"K": K, "want_grad": want_grad, "api": _compare(api_sweep, api_loop, reps)}
            # the launches alone, through the C ABI, on the buffers the engine just used
            prob, L = eng.prob, levels.shape[1]
            ng = L if want_grad else 0
            n_part = lib.nic_closed_form_num_partials(prob.B, prob.S)
            part_k, part_1 = torch.empty(K, n_part, ng + 2, device=dev), torch.empty(n_part, ng + 2, device=dev)
            desc = closed_form.make_desc(prob, policy_name, T, 0, 0, rows[0], sc.demands_soa, eng.state0)
            descs = [closed_form.make_desc(prob, policy_name, T, 0, 0, row, sc.demands_soa, eng.state0) for row in rows]
            stream = _lib.current_stream()

            def abi_sweep():
                _lib.check(lib.nic_closed_form_sweep(desc, levels.data_ptr(), K, None, part_k.data_ptr(), ng + 2, int(want_grad), stream))

            def abi_loop():
                for d in descs:
                    _lib.check(lib.nic_closed_form_rollout_sums(d, None, None, None, part_1.data_ptr(), ng + 2, int(want_grad), 1, stream))
            abi_loop()
            case["single_kernel"] = (lib.nic_last_kernel() or b"").decode()
            abi_sweep()
            case["sweep_kernel"] = (lib.nic_last_kernel() or b"").decode()
            case["kernel"] = _compare(abi_sweep, abi_loop, reps)
            # same numbers on both sides (per-wavefront rows are equal bit for bit; here the last candidate's, which the loop left behind)
            case["last_candidate_rows_equal"] = bool(torch.equal(part_k[K - 1], part_1))
            out["cases"].append(case)
            print(json.dumps({"policy": policy_name, **{k: v for k, v in case.items()}}), flush=True)
    del model.closed_form_levels
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scenarios", type=int, default=32768)
    ap.add_argument("--periods", type=int, default=100)
    ap.add_argument("--candidates", type=int, nargs="+", default=[16, 64])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--policies", nargs="+", default=["base_stock", "capped_base_stock", "echelon_stock"])
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--lib", default=None, help="another build of libnic_hip.so to time")
    args = ap.parse_args()
    from neural_inventory_control_amd import _lib
    if args.lib:
        _lib.LIB_PATH = os.path.abspath(args.lib)
    _lib.require_device()
    os.makedirs(args.out_dir, exist_ok=True)
    for name in args.policies:
        res = measure(name, args.scenarios, args.periods, args.candidates, args.reps)
        with open(os.path.join(args.out_dir, f"closed_form_sweep_{name}.json"), "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
