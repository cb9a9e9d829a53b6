#!/usr/bin/env python
"""Training step of a bench workload with the MLP engine's GEMMs in FP32 (the default) and in bf16 (FusedRollout.gemm_precision =
"bf16", csrc/linear_bf16.hip), both in one process: rollout forward + backward + Adam between two synchronises, the median of
--steps after --warmup.  Then one eager step per precision under a KernelTimer (every launch bracketed) for per-kernel averages.
Prints one JSON line; the bf16 GEMMs are graded against HBM bytes (with FP32 activations they are bandwidth-bound, not MFMA-bound).

    python tools/bf16_step.py --workload cfg3 [--steps 10 --warmup 3] [--scenarios N --periods T] [--out profiles/x.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
from neural_inventory_control_amd.rollout import KernelTimer  # noqa: E402

HBM_PEAK = 8.0e12   # MI355X HBM3E, bytes/s (MI355X_MICROARCH.md)


def hbm_bytes(tag, n, T):
    """algorithmic HBM bytes per launch of a bf16 GEMM tag at n scenarios: FP32 activations read / written once, weights ignored"""
    N, K = (int(v) for v in tag.rsplit("_", 1)[1].split("x"))
    if tag.startswith("fwd_bf16"):
        return 4 * n * (K + N)                 # X in, Y out
    if tag.startswith("dgrad_bf16"):
        return 4 * n * (N + 2 * K)             # dY in, Hprev in, dX out
    if tag.startswith("wgradT_bf16"):
        return 4 * n * T * (N + K)             # dZ and X histories of every period
    if tag.startswith("wgrad_bf16"):
        return 4 * n * (N + K)
    return None


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--workload", default="cfg3")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--scenarios", type=int, default=None)
    ap.add_argument("--periods", type=int, default=None)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    setting, policy, sc, data, model, eng, n, T, desc = bench.build_case(args.workload, dev, 0, 1, args.scenarios, args.periods)
    if eng is None or not hasattr(eng, "gemm_precision"):
        raise SystemExit(f"{args.workload}: not a workload of the fused MLP engine")
    obs = setting["observation_params"]
    eng.materialize(eng.input_rows(data, obs))   # (lazy first layer: materialised before the weights are snapshotted)
    opt = torch.optim.Adam(model.parameters(), lr=3e-4)
    init = {k: v.detach().clone() for k, v in model.state_dict().items()}
    out = {"tool": "bf16_step", "workload": args.workload, "desc": desc, "n_scenarios": n, "periods": T,
           "library_id": bench._lib_id() or None, "gpu": torch.cuda.get_device_name(dev), "ms_per_step": {}, "kernels": {},
           "bf16_layers": None}

    def step():
        opt.zero_grad(set_to_none=False)
        eng.run(data, T, 0, train=True, observation_params=obs, demand_soa=sc.demands_soa)
        opt.step()

    for precision in ("fp32", "bf16"):
        model.load_state_dict(init)   # (same weights for both precisions)
        eng.gemm_precision = precision
        for _ in range(max(args.warmup, 1)):
            step()
        times = []
        for _ in range(args.steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            step()
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) * 1e3)
        out["ms_per_step"][precision] = round(statistics.median(times), 3)
        timer = eng.timer = KernelTimer(stride=1)
        step()
        torch.cuda.synchronize()
        eng.timer = None
        ks = {}
        for tag, (calls, ms) in sorted(timer.summary().items()):
            e = {"launches": calls, "mean_ms": round(ms, 5), "kernel": timer.names.get(tag)}
            b = hbm_bytes(tag, n, T) if "_bf16_" in tag else None
            if b is not None:
                e["hbm_bytes_per_launch"] = b
                e["achieved_tb_s"] = round(b / (ms * 1e-3) / 1e12, 3)
                e["frac_of_hbm_peak"] = round(b / (ms * 1e-3) / HBM_PEAK, 3)
            ks[tag] = e
        out["kernels"][precision] = ks
        if precision == "bf16":
            out["bf16_layers"] = list(eng.bf16_layers)
    out["speedup"] = round(out["ms_per_step"]["fp32"] / out["ms_per_step"]["bf16"], 3)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
