"""What the host and the GPU tests of the ensemble Adam share: the inputs, the stand-alone host build of
csrc/ensemble_adam_body.h (tests/ensemble_adam_harness.cpp, the kernels' referee bit for bit) and the float64 Adam both are held to."""
import os
import shutil
import subprocess

import numpy as np

from neural_inventory_control_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (lr, beta1, beta2, eps, weight_decay) of the three models
HYPER = [(1e-2, 0.9, 0.999, 1e-8, 0.0), (3e-3, 0.8, 0.99, 1e-6, 1e-2), (1e-3, 0.95, 0.9995, 1e-8, 0.0)]
STEPS = 5
STATE_DTYPE = np.dtype([("step", "<i4"), ("reserved", "<i4"), ("c1", "<f8"), ("c2", "<f8")])   # NicEnsembleAdamState
N_COEF = 8


def inputs(P, K=3, steps=STEPS):
    """parameters uniform in +-0.5; gradients randn x 10^U(-4, 2) with every 7th element exactly 0 (no denormals anywhere in five
    steps: the smallest non-zero v is (1 - beta2) g^2 >~ 1e-4 x 1e-20)"""
    rng = np.random.RandomState(20240 + P)
    params = rng.uniform(-0.5, 0.5, size=(K, P)).astype(np.float32)
    grads = (rng.standard_normal((steps, K, P)) * 10.0 ** rng.uniform(-4, 2, size=(steps, K, P))).astype(np.float32)
    grads.reshape(steps, -1)[:, ::7] = 0.0
    return params, grads, np.array(HYPER[:K], dtype=np.float64)


def host_compiler():
    hipcc = os.path.realpath(shutil.which(build._hipcc()) or build._hipcc())
    for c in (os.path.join(os.path.dirname(hipcc), "..", "llvm", "bin", "clang++"), "/opt/rocm/llvm/bin/clang++",
              shutil.which("clang++"), shutil.which("g++")):
        if c and os.path.isfile(c):
            return c
    raise RuntimeError("no host C++ compiler to build tests/ensemble_adam_harness.cpp")


def build_harness(directory):
    """(-Wall -Werror: the header has to stay clean C++ for a compiler that knows nothing of HIP; -ffp-contract=off as the kernels)"""
    exe = os.path.join(str(directory), "ensemble_adam_harness")
    subprocess.run([host_compiler(), "-O1", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-o", exe,
                    os.path.join(ROOT, "tests", "ensemble_adam_harness.cpp")], check=True)
    return exe


def padded(a, stride, fill=np.nan):
    """[..., P] -> [..., stride] with `fill` past column P"""
    out = np.full(a.shape[:-1] + (stride,), fill, dtype=np.float32)
    out[..., :a.shape[-1]] = a
    return out


def fresh_state(K):
    st = np.zeros(K, dtype=STATE_DTYPE)
    st["c1"] = st["c2"] = 1.0
    return st


def run_harness(exe, directory, P, params, grads, hyper, exp_avg, exp_avg_sq, state):
    """params [K][ps], grads [steps][K][gs], exp_avg [K][es], exp_avg_sq [K][vs] (float32, any strides >= P), state [K] ->
    dict(params, exp_avg, exp_avg_sq, state, coef) after grads.shape[0] steps"""
    K, steps = params.shape[0], grads.shape[0]
    ps, gs, es, vs = params.shape[1], grads.shape[2], exp_avg.shape[1], exp_avg_sq.shape[1]
    src, dst = os.path.join(str(directory), "in.bin"), os.path.join(str(directory), "out.bin")
    with open(src, "wb") as f:
        f.write(np.array([K, P, steps, ps, gs, es, vs], dtype="<i8").tobytes())
        for a in (hyper.astype("<f8"), state.astype(STATE_DTYPE), params, grads, exp_avg, exp_avg_sq):
            f.write(np.ascontiguousarray(a).tobytes())
    subprocess.run([exe, "run", src, dst], check=True)
    raw = open(dst, "rb").read()
    out, off = {}, 0
    for name, shape, dt in (("params", (K, ps), "<f4"), ("exp_avg", (K, es), "<f4"), ("exp_avg_sq", (K, vs), "<f4"),
                            ("state", (K,), STATE_DTYPE), ("coef", (K, N_COEF), "<f4")):
        n = int(np.prod(shape)) * np.dtype(dt).itemsize
        out[name] = np.frombuffer(raw[off:off + n], dtype=dt).reshape(shape).copy()
        off += n
    assert off == len(raw)
    return out


def adam_f64(params, grads, hyper, m0=None, v0=None, t0=0):
    """the referee: Adam in float64 with beta ** t, on the float32 inputs (from the moments m0, v0 after t0 steps, if given)"""
    p = params.astype(np.float64)
    m = np.zeros_like(p) if m0 is None else m0.astype(np.float64)
    v = np.zeros_like(p) if v0 is None else v0.astype(np.float64)
    lr, b1, b2, eps, wd = (hyper[:, i:i + 1] for i in range(5))
    for t in range(t0 + 1, t0 + grads.shape[0] + 1):
        g = grads[t - t0 - 1].astype(np.float64)
        g = np.where(wd != 0, g + wd * p, g)
        m = b1 * m + (1 - b1) * g
        v = b2 * v + (1 - b2) * g * g
        p = p - lr / (1 - b1 ** t) * (m / (np.sqrt(v) / np.sqrt(1 - b2 ** t) + eps))
    return p


def torch_adam(params, grads, hyper_row):
    """default torch.optim.Adam (CPU, float32) on one model's row -> its parameters after grads.shape[0] steps"""
    import torch
    p = torch.nn.Parameter(torch.from_numpy(params.copy()))
    lr, b1, b2, eps, wd = (float(x) for x in hyper_row)
    opt = torch.optim.Adam([p], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
    for g in grads:
        p.grad = torch.from_numpy(g.copy())
        opt.step()
    return p.detach().numpy(), opt


def bits(a):
    return np.ascontiguousarray(a).view(np.int32 if a.dtype == np.float32 else np.uint8)
