"""Records what the forward / input-gradient dispatch (csrc/wx_plan.h behind nic_linear_fwd, nic_linear_dgrad) DOES, so that a
change that must not move it can be held to the record.

    python tools/record_wx_pins.py --grid                                    # the cases of the table, one "M K ncols operands_ok" per line
    python tools/record_wx_pins.py --gpu tests/golden/wx_dispatch_pins.json  # MI355X; run twice and compare the files

--grid: tests/golden/wx_plan_cu256.txt was made from these lines at the commit BEFORE the dispatch moved into the header: that
        commit's pick_wx_tile, pick_wx_stream and the two switch ladders of dispatch_wx, copied unchanged into a scratch program
        (not kept) with nic::cu_count() replaced by 256, which read the lines and appended to each the kernel the ladder reached
        (template name and arguments, without the epilogue), its grid and its block size.
--gpu:  run at a PARENT commit (check the parent out, build it, copy this script into its tools/): for every case of PIN_CASES,
        forward and input gradient, the kernel nic_last_kernel() names after the call and the SHA-256 of the output matrix, its
        NaN-filled padding columns included.
tests/test_wx_plan_host.py and tests/test_gpu_kernels.py read the two files and take the cases from here."""
import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# ---- plan table --------------------------------------------------------------------------------------------------------------
# both sides of every threshold of the pickers at 256 compute units.  For M = 512: 32 x 32 tiles <= 512 up to 1,024 columns (KS = 4),
# 1,056 columns = 528 tiles (KS = 2), 2,048 = 1,024 tiles (the last streamed count), 2,080 = 1,040 (the first LDS-DMA count),
# 16,256 = 508 tiles of 128 x 128, 16,384 = 512 (the first 128 x 128 launch)
GRID_MS = [1, 17, 32, 33, 64, 65, 128, 129, 195, 256, 393, 512, 1024]
GRID_KS = [16, 64, 127, 128, 255, 256, 512]
GRID_NCOLS = [4, 36, 64, 128, 132, 256, 512, 1024, 1056, 2048, 2080, 4096, 8192, 16256, 16384, 32768, 65536]


def plan_grid():
    return [(M, K, n, ok) for M in GRID_MS for K in GRID_KS for n in GRID_NCOLS for ok in (1, 0)]


# ---- dispatch pins -----------------------------------------------------------------------------------------------------------
# (id, rows out, contraction, scenarios, weight layout): the smallest shape that reaches each branch on 256 compute units.  Layout
# "padded": row stride a multiple of 32 floats, 16-byte aligned; "ragged": unpadded, row stride = contraction (51: not a multiple
# of 4); "offset": the weight starts one float off a 16-byte boundary, row stride 68
PIN_CASES = [
    ("stream_ks2", 17, 128, 64, "padded"),
    ("stream_ks4", 17, 512, 64, "padded"),
    ("stream_ks2_many_tiles", 512, 512, 1056, "padded"),
    ("dma_after_stream_cutoff", 512, 512, 2080, "padded"),
    ("dma_64x128", 64, 64, 128, "padded"),
    ("dma_32x128", 17, 64, 128, "padded"),
    ("dma_32x128_ragged", 393, 64, 132, "padded"),
    ("dma_128x128", 512, 32, 16384, "padded"),
    ("staged_128x128", 65, 51, 100, "ragged"),
    ("staged_64x128", 33, 51, 100, "ragged"),
    ("staged_32x256", 17, 51, 100, "ragged"),
    ("staged_by_address", 64, 64, 128, "offset"),
]
# (case id, direction): "fwd" = linear_fwd with bias and ELU, "dgrad" = linear_dgrad with Hprev and ELU, "dgrad_accumulate" = the
# same added to a filled dX
PIN_RUNS = [(c[0], d) for c in PIN_CASES for d in ("fwd", "dgrad")] + [("dma_64x128", "dgrad_accumulate")]
PIN_IDS = [f"{c}-{d}" for c, d in PIN_RUNS]


def case_operands_ok(case):
    return case[4] == "padded"


def run_pin_case(case_id, direction, dev="cuda"):
    """-> {"kernel": name of the kernel of the call, "sha256": of the output [rows out][ldb], NaN padding columns included}"""
    import torch
    from neural_inventory_control_amd import _lib, ops
    case = next(c for c in PIN_CASES if c[0] == case_id)
    _, M, K, B, layout = case
    gen = torch.Generator().manual_seed(2000 + 10 * PIN_CASES.index(case) + (direction != "fwd"))
    ldb = (B + 3) // 4 * 4 + 8
    lda = {"padded": (K + 31) // 32 * 32, "ragged": K, "offset": K + 4}[layout]
    off = 1 if layout == "offset" else 0
    flat = (torch.randn(M * lda + 4, generator=gen) * 0.3).to(dev)   # (torch allocations are 16-byte aligned and more)
    A = flat[off:off + M * lda].view(M, lda)[:, :K]
    Bm = torch.randn(K, ldb, generator=gen).to(dev)
    out = torch.full((M, ldb), float("nan"), device=dev)
    if direction == "fwd":
        bias = torch.randn(M, generator=gen).to(dev)
        ops.linear_fwd(A, bias, Bm, out, B, _lib.NIC_ACT_ELU)
    else:
        H = torch.randn(M, ldb, generator=gen).to(dev)
        if direction == "dgrad_accumulate":
            out[:, :(B + 3) // 4 * 4] = torch.randn(M, (B + 3) // 4 * 4, generator=gen).to(dev)
        ops.linear_dgrad(A, Bm, H, out, B, _lib.NIC_ACT_ELU, direction == "dgrad_accumulate")
    kernel = _lib.lib().nic_last_kernel().decode()
    torch.cuda.synchronize()
    return {"kernel": kernel, "sha256": hashlib.sha256(out.cpu().numpy().tobytes()).hexdigest()}


def record_pins(path):
    pins = {f"{c}-{d}": run_pin_case(c, d) for c, d in PIN_RUNS}
    with open(path, "w") as f:
        json.dump(pins, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--grid", action="store_true")
    ap.add_argument("--gpu", metavar="OUT")
    args = ap.parse_args()
    if args.grid:
        for row in plan_grid():
            print(*row)
    if args.gpu:
        record_pins(args.gpu)
