"""What the host and the GPU tests of the clipped ensemble Adam share: the per-model max norms, the stand-alone host build of
csrc/ensemble_clip_body.h (tests/ensemble_clip_harness.cpp, the kernels' referee bit for bit), the float64 clip + Adam both are held
to and torch's own `clip_grad_norm_` + Adam as the yardstick.  Inputs, padding and the state layout are ensemble_adam_checks'."""
import os
import subprocess

import numpy as np

import ensemble_adam_checks as eac

ROOT = eac.ROOT
MAX_NORMS = (float("inf"), 1.0, 1e6)   # per model: not clipped; clipped at these gradients' sizes; finite and never reached
N_CLIP = 2                             # floats of a model's clip row {scale, norm} (csrc/ensemble_clip_body.h: EcClip)
NORM_EPS = 1e-6                        # torch.nn.utils.clip_grad_norm_'s


def build_harness(directory):
    """(-Wall -Werror: the header has to stay clean C++ for a compiler that knows nothing of HIP; -ffp-contract=off as the kernels)"""
    exe = os.path.join(str(directory), "ensemble_clip_harness")
    subprocess.run([eac.host_compiler(), "-O1", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-o", exe,
                    os.path.join(ROOT, "tests", "ensemble_clip_harness.cpp")], check=True)
    return exe


def run_harness(exe, directory, P, params, grads, hyper, max_norm, exp_avg, exp_avg_sq, state):
    """params [K][ps], grads [steps][K][gs], exp_avg [K][es], exp_avg_sq [K][vs] (float32, any strides >= P), max_norm [K], state [K]
    -> dict(params, exp_avg, exp_avg_sq, state, coef, clip [steps][K][2]) after grads.shape[0] steps"""
    K, steps = params.shape[0], grads.shape[0]
    ps, gs, es, vs = params.shape[1], grads.shape[2], exp_avg.shape[1], exp_avg_sq.shape[1]
    src, dst = os.path.join(str(directory), "in.bin"), os.path.join(str(directory), "out.bin")
    with open(src, "wb") as f:
        f.write(np.array([K, P, steps, ps, gs, es, vs], dtype="<i8").tobytes())
        for a in (hyper.astype("<f8"), np.asarray(max_norm, dtype="<f8"), state.astype(eac.STATE_DTYPE), params, grads, exp_avg, exp_avg_sq):
            f.write(np.ascontiguousarray(a).tobytes())
    subprocess.run([exe, "run", src, dst], check=True)
    raw = open(dst, "rb").read()
    out, off = {}, 0
    for name, shape, dt in (("params", (K, ps), "<f4"), ("exp_avg", (K, es), "<f4"), ("exp_avg_sq", (K, vs), "<f4"),
                            ("state", (K,), eac.STATE_DTYPE), ("coef", (K, eac.N_COEF), "<f4"), ("clip", (steps, K, N_CLIP), "<f4")):
        n = int(np.prod(shape)) * np.dtype(dt).itemsize
        out[name] = np.frombuffer(raw[off:off + n], dtype=dt).reshape(shape).copy()
        off += n
    assert off == len(raw)
    return out


def norms_f64(grads):
    """[..., P] float32 -> [...] float64 L2 norms"""
    return np.sqrt((grads.astype(np.float64) ** 2).sum(axis=-1))


def scales_f64(norms, max_norm):
    """clip_grad_norm_'s factor in float64; max_norm broadcasts against norms"""
    max_norm = np.broadcast_to(np.asarray(max_norm, dtype=np.float64), norms.shape)
    with np.errstate(invalid="ignore"):
        return np.where(np.isinf(max_norm), 1.0, np.minimum(1.0, max_norm / (norms + NORM_EPS)))


def clipped_f64(grads, max_norm):
    """[steps][K][P] float32 -> the clipped gradients in float64"""
    return grads.astype(np.float64) * scales_f64(norms_f64(grads), max_norm)[..., None]


def clip_adam_f64(params, grads, hyper, max_norm, m0=None, v0=None, t0=0):
    """the referee: clipping and Adam in float64 on the float32 inputs.  (eac.adam_f64 takes the gradients through float64 whatever
    their type.)"""
    return eac.adam_f64(params, clipped_f64(grads, max_norm), hyper, m0, v0, t0)


def torch_clip_adam(params, grads, hyper_row, max_norm):
    """torch's own route on one model's row (CPU, float32): clip_grad_norm_ then a default torch.optim.Adam, grads.shape[0] steps ->
    (parameters, the norms clip_grad_norm_ returned)"""
    import torch
    p = torch.nn.Parameter(torch.from_numpy(params.copy()))
    lr, b1, b2, eps, wd = (float(x) for x in hyper_row)
    opt = torch.optim.Adam([p], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
    norms = []
    for g in grads:
        p.grad = torch.from_numpy(g.copy())
        norms.append(float(torch.nn.utils.clip_grad_norm_([p], max_norm)))
        opt.step()
    return p.detach().numpy(), norms


def ulps32(got, want64):
    """|got - want| in units of float32 spacing at want (got float32, want float64)"""
    want64 = np.asarray(want64, dtype=np.float64)
    return np.abs(np.asarray(got, dtype=np.float64) - want64) / np.spacing(np.abs(want64).astype(np.float32)).astype(np.float64)
