"""Opt-in bf16 GEMMs (csrc/linear_bf16.hip), the parts that need no GPU: the FP32 -> bf16 rounding helper against torch bit for
bit, the compiled kernels' instructions, and the `gemm_precision` setting from main_run down to the engine."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from neural_inventory_control_amd import build, main_run, workloads  # noqa: E402
from neural_inventory_control_amd.rollout import check_gemm_precision  # noqa: E402
from neural_inventory_control_amd.trainer import Trainer  # noqa: E402

SRC = os.path.join(ROOT, "neural_inventory_control_amd", "csrc", "linear_bf16.hip")


def _host_clang():
    """clang++ next to hipcc (the helper uses the __bf16 type, which needs a clang host compiler), else one on PATH"""
    hipcc = os.path.realpath(shutil.which(build._hipcc()) or build._hipcc())
    for c in (os.path.join(os.path.dirname(hipcc), "..", "llvm", "bin", "clang++"), "/opt/rocm/llvm/bin/clang++",
              shutil.which("clang++")):
        if c and os.path.isfile(c):
            return c
    raise RuntimeError("no clang++ to build the host harness of csrc/nic_bf16.h")


@pytest.fixture(scope="module")
def to_bf16(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("bf16") / "harness.so")
    subprocess.run([_host_clang(), "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so,
                    os.path.join(ROOT, "tests", "bf16_convert_harness.cpp")], check=True)
    lib = ctypes.CDLL(so)
    lib.nic_test_f32_to_bf16.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]

    def run(bits):
        bits = np.ascontiguousarray(bits, dtype=np.uint32)
        out = np.empty(bits.shape, dtype=np.uint16)
        lib.nic_test_f32_to_bf16(bits.ctypes.data, out.ctypes.data, bits.size)
        return out
    return run


def _torch_bf16(bits):
    f = torch.from_numpy(np.ascontiguousarray(bits, dtype=np.uint32).view(np.float32))
    return f.to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)


def _is_nan_bf16(b):
    return ((b & 0x7F80) == 0x7F80) & ((b & 0x7F) != 0)


def _compare(to_bf16, bits):
    got, want = to_bf16(bits), _torch_bf16(bits)
    nan_in = np.isnan(np.ascontiguousarray(bits, dtype=np.uint32).view(np.float32))
    assert _is_nan_bf16(got[nan_in]).all(), "NaN in must give NaN out"
    ok = got[~nan_in] == want[~nan_in]
    bad = np.flatnonzero(~ok)
    assert ok.all(), [(hex(int(bits[~nan_in][i])), hex(int(got[~nan_in][i])), hex(int(want[~nan_in][i]))) for i in bad[:8]]


def test_rounding_random_patterns(to_bf16):
    rng = np.random.default_rng(0)
    _compare(to_bf16, rng.integers(0, 2 ** 32, size=2 ** 24, dtype=np.uint64).astype(np.uint32))


def test_rounding_every_tie(to_bf16):
    # low 16 bits exactly 0x8000: halfway between two bf16 values, for every upper half (both signs, all exponents incl. inf/NaN)
    bits = (np.arange(2 ** 16, dtype=np.uint32) << 16) | 0x8000
    _compare(to_bf16, bits)
    # ... and one ulp of FP32 either side of every tie
    _compare(to_bf16, bits - 1)
    _compare(to_bf16, bits + 1)


def test_rounding_special_values(to_bf16):
    specials = np.array([0x00000000, 0x80000000,                 # +-0
                         0x00000001, 0x00008000, 0x00018000, 0x007FFFFF, 0x807FFFFF, 0x00800000,   # subnormals, smallest normal
                         0x7F800000, 0xFF800000,                 # +-inf
                         0x7F7FFFFF, 0xFF7FFFFF,                 # largest finite (rounds to inf)
                         0x7FC00000, 0xFFC00000, 0x7FFFFFFF,     # quiet NaNs
                         0x7F800001, 0x7FA00000, 0xFF800001,     # signalling NaNs
                         0x7F808000, 0x7F80FFFF], dtype=np.uint32)   # NaNs whose payload sits below the bf16 mantissa
    _compare(to_bf16, specials)
    got = to_bf16(specials)
    assert got[0] == 0x0000 and got[1] == 0x8000 and got[8] == 0x7F80 and got[9] == 0xFF80
    assert _is_nan_bf16(got[12:]).all()


def _kernels(asm_text):
    """{kernel symbol: [instruction lines]} of a gfx950 device assembly listing"""
    out, cur = {}, None
    for line in asm_text.splitlines():
        m = re.match(r"^(_Z\w+):", line)
        if m:
            cur = out.setdefault(m.group(1), [])
            continue
        if cur is not None and line.startswith("\t.size"):
            cur = None
        if cur is not None:
            cur.append(line.split(";")[0].rstrip())
    return out


@pytest.fixture(scope="module")
def asm_path():
    import isa_asm_audit
    return isa_asm_audit.compile_to_asm(SRC, [])


def test_isa_bf16_mfma_and_no_scratch_in_k_loops(asm_path):
    kernels = {k: v for k, v in _kernels(open(asm_path).read()).items() if "bf16_" in k and "_kernel" in k}
    assert len(kernels) >= 5, sorted(kernels)   # forward x 2 tilings, dgrad x 2 tilings, weight gradient
    for name, lines in kernels.items():
        assert any("v_mfma_f32_32x32x16_bf16" in ln or "v_mfma_f32_16x16x32_bf16" in ln for ln in lines), name
        labels = {ln.strip()[:-1]: i for i, ln in enumerate(lines) if re.match(r"^\.?\w+:$", ln.strip())}
        loops = 0
        for i, ln in enumerate(lines):
            m = re.match(r"\s*s_(?:cbranch_\w+|branch)\s+(\S+)", ln)
            if m and m.group(1) in labels and labels[m.group(1)] < i:   # a backward branch: the body is target .. branch
                body = lines[labels[m.group(1)]:i + 1]
                if any("v_mfma" in b for b in body):
                    loops += 1
                    assert not any("scratch_" in b for b in body), f"{name}: scratch access inside a k loop"
        assert loops >= 1, f"{name}: no k loop with MFMAs found"


def test_isa_asm_audit_clean(asm_path):
    import isa_asm_audit
    _, _, problems = isa_asm_audit.audit(asm_path)
    assert problems == []


def test_precision_setting_defaults_and_validation():
    assert Trainer().gemm_precision == "fp32"
    assert check_gemm_precision("fp32") == "fp32" and check_gemm_precision("bf16") == "bf16"
    for bad in ("fp16", "BF16", "", None, 16):
        with pytest.raises(ValueError):
            check_gemm_precision(bad)


def _built(precision):
    setting, hyper, _ = workloads.get_epoch("cfg3_yaml")
    for ds in setting["params_by_dataset"].values():   # (small datasets: only the trainer's settings are under test)
        ds["n_samples"] = ds["batch_size"] = 64
        ds["periods"] = 4
        ds["ignore_periods"] = 0
    if precision is not None:
        hyper["trainer_params"]["gemm_precision"] = precision
    return main_run.build(setting, hyper, "cpu")


def test_main_run_passes_gemm_precision():
    assert _built(None)["trainer"].gemm_precision == "fp32"   # the reference's YAML files have no such key
    assert _built("bf16")["trainer"].gemm_precision == "bf16"
    with pytest.raises(ValueError):
        _built("fp8")
