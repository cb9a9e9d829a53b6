"""Records what the weight-gradient dispatch (csrc/wgrad_plan.h behind nic_linear_wgrad*, nic_wgrad*_num_splits) DOES, so that a
change that must not move it can be held to the record.  Run it at a PARENT commit (check the parent out, build it, copy this
script into its tools/), then commit the files it wrote with the change:

    python tools/record_wgrad_pins.py --slots tests/golden/wgrad_slots_cu256.txt     # no GPU needed: 256 CUs assumed without one
    python tools/record_wgrad_pins.py --gpu tests/golden/wgrad_dispatch_pins.json    # MI355X; run twice and compare the files

--slots: nic_wgrad_num_splits and nic_wgrad_periods_num_splits over SLOT_GRID, one line of integers per (N, K, B):
         N K B single-period-slots, then the all-period slots for every T of SLOT_TS.
--gpu:   for every case of PIN_CASES the kernel nic_last_kernel() names after the call, the number of slab slots with a non-zero
         entry, and the SHA-256 of dW and db after wgrad_reduce.
tests/test_wgrad_plan_host.py and tests/test_gpu_kernels.py read the two files and take the cases from here."""
import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# ---- slot table ------------------------------------------------------------------------------------------------------------------
# both sides of every threshold of the classifiers and slot functions
SLOT_NS = [1, 17, 31, 32, 33, 64, 65, 95, 96, 128, 129, 191, 192, 300, 383, 384, 512]
SLOT_KS = [4, 26, 32, 33, 51, 64, 65, 96, 100, 128, 129, 191, 192, 256, 257, 393, 448, 449, 512]
SLOT_BS = [63, 72, 100, 128, 256, 300, 1024, 1056, 8192, 65536]
SLOT_TS = [1, 2, 7, 100, 3, 4, 5, 6, 9, 10, 19]   # (the first four: the grid; the rest: horizons of the GPU tests' cases)
# the (N, K, B) of test_linear_wgrad_periods_* and THIN_SHAPES (tests/test_gpu_kernels.py)
SLOT_EXTRA = [(512, 512, 2048), (256, 200, 1024), (300, 512, 1056), (64, 33, 100),
              (512, 512, 1024), (512, 512, 256), (512, 51, 1024), (512, 51, 512), (98, 512, 512), (512, 393, 384), (512, 512, 8192),
              (512, 66, 1024), (320, 150, 512), (64, 597, 72), (66, 64, 72), (64, 64, 100), (200, 100, 300),
              (17, 512, 777), (17, 512, 4096), (5, 128, 130), (32, 256, 1000), (1, 32, 64), (18, 96, 2049), (9, 64, 63)]


def slot_grid():
    return [(N, K, B) for N in SLOT_NS for K in SLOT_KS for B in SLOT_BS] + SLOT_EXTRA


def record_slots(path):
    from neural_inventory_control_amd import ops
    with open(path, "w") as f:
        f.write("# N K B nic_wgrad_num_splits, then nic_wgrad_periods_num_splits for T = " + " ".join(map(str, SLOT_TS)) +
                "  (256 compute units; tools/record_wgrad_pins.py --slots)\n")
        for N, K, B in slot_grid():
            row = [N, K, B, ops.wgrad_num_splits(N, K, B)] + [ops.wgrad_periods_num_splits(N, K, B, T) for T in SLOT_TS]
            f.write(" ".join(map(str, row)) + "\n")


# ---- dispatch pins ---------------------------------------------------------------------------------------------------------------
# (id, entry, N, K, B, T, slots): entry "one" = linear_wgrad, "periods" = linear_wgrad_periods, "one_unaligned" = linear_wgrad on
# operands 4 bytes off a 16-byte boundary, "bf16_one" / "bf16_periods" = the bf16 entries; slots None = the count the library asks
# for.  The smallest shapes that reach each branch of the plan.
PIN_CASES = [
    ("dma_big", "periods", 512, 512, 256, 3, None),
    ("dma_tall", "periods", 512, 51, 256, 3, None),
    ("dma_half", "periods", 512, 66, 256, 2, None),
    ("dma_mid", "periods", 98, 512, 256, 3, None),
    ("dma_wide", "periods", 512, 393, 128, 2, None),
    ("dma_big_one_period", "one", 256, 200, 1024, 1, None),
    ("dma_big_periods_entry_T1", "periods", 256, 200, 1024, 1, None),
    ("dma_odd_slots", "periods", 512, 512, 256, 9, 7),
    ("staged_128x128_ragged", "one", 200, 100, 300, 1, None),
    ("staged_128x64", "one", 128, 7, 777, 1, None),
    ("staged_64x128", "one", 64, 64, 64, 1, None),
    ("staged_32x256_thin", "one", 17, 512, 777, 1, None),
    ("staged_unaligned", "one_unaligned", 200, 100, 300, 1, 3),
    ("dma_shape_ragged_scenarios", "periods", 512, 512, 100, 2, None),
    ("small_k26", "one", 5, 26, 300, 1, None),
    ("small_k96", "one", 17, 96, 1000, 1, None),
    ("periods_per_period_small", "periods", 32, 4, 100, 3, None),
    ("periods_one_launch_pairs", "periods", 64, 64, 72, 10, None),
    ("periods_pairs_odd_slots", "periods", 64, 64, 100, 7, 5),
    ("periods_per_group_one_launch", "periods", 200, 100, 300, 19, 1),
    ("periods_per_group_4_3", "periods", 66, 64, 2000, 7, 1),
    ("periods_per_group_small_rest", "periods", 17, 96, 2048, 5, 1),
    ("bf16_one", "bf16_one", 160, 224, 300, 1, 3),
    ("bf16_periods", "bf16_periods", 160, 224, 300, 7, 6),
]


def run_pin_case(case, dev="cuda"):
    """-> {"kernel": name of the last kernel of the call, "used_slots": slab slots with a non-zero entry, "sha256": of dW, db}"""
    import torch
    from neural_inventory_control_amd import _lib, ops
    name, entry, N, K, B, T, slots = case
    gen = torch.Generator().manual_seed(1000 + PIN_CASES.index(case))
    ldb = (B + 3) // 4 * 4 + 8
    lds = (K + 1 + 3) // 4 * 4
    off = 1 if entry == "one_unaligned" else 0

    def operand(rows):   # [T][rows][ldb] from the seeded CPU generator (`off` floats into a 16-byte aligned block)
        flat = torch.randn(T * rows * ldb + 4, generator=gen).to(dev)
        return flat[off:off + T * rows * ldb].view(T, rows, ldb)
    dY, X = operand(N), operand(K)
    if slots is None:
        slots = ops.wgrad_periods_num_splits(N, K, B, T) if entry == "periods" else ops.wgrad_num_splits(N, K, B)
    slab = torch.zeros(slots, N, lds, device=dev)
    if entry in ("one", "one_unaligned"):
        ops.linear_wgrad(dY[0], X[0], slab, B)
    elif entry == "periods":
        ops.linear_wgrad_periods(dY, X, slab, B)
    elif entry == "bf16_one":
        ops.linear_bf16_wgrad(dY[0], X[0], slab, B)
    else:
        ops.linear_bf16_wgrad_periods(dY, X, slab, B)
    kernel = _lib.lib().nic_last_kernel().decode()
    dW = torch.full((N, K), float("nan"), device=dev)
    db = torch.full((N,), float("nan"), device=dev)
    ops.wgrad_reduce(slab, dW, db, K, 1.0)
    torch.cuda.synchronize()
    h = hashlib.sha256()
    h.update(dW.cpu().numpy().tobytes())
    h.update(db.cpu().numpy().tobytes())
    return {"kernel": kernel, "used_slots": int((slab.abs().sum(dim=(1, 2)) > 0).sum()), "sha256": h.hexdigest()}


def record_pins(path):
    pins = {case[0]: run_pin_case(case) for case in PIN_CASES}
    with open(path, "w") as f:
        json.dump(pins, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--slots", metavar="OUT")
    ap.add_argument("--gpu", metavar="OUT")
    args = ap.parse_args()
    if args.slots:
        record_slots(args.slots)
    if args.gpu:
        record_pins(args.gpu)
