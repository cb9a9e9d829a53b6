"""`EnsembleAdam`: Adam for K models whose parameters are the rows of one [K][P] buffer, stepped by two launches for all of them
(`nic_ensemble_adam_prepare` / `_update`, csrc/ensemble_adam.hip; the arithmetic is csrc/ensemble_adam_body.h's).  Replaces K
`torch.optim.Adam` objects, or one with K parameter groups (main_run.py:110's optimizer, trainer.py:177's `optimizer.step()`), behind
`SmallPolicyEnsemble.train_step`.

The hyper-parameters and the step counters live on the device: the kernels read them, so a captured step sees a scheduler's
`set_lr` and advances its own counters.  The bias corrections come from running products c1 = beta1^t, c2 = beta2^t kept in double
next to the counter (no `pow`: host and device maths libraries differ on it, double `*` does not).  No amsgrad, no `maximize`.

`max_grad_norm` clips every model's total gradient norm inside the same two launches (trainer.py:175-176's `clip_grad_norm_`, per
model; `nic_ensemble_adam_prepare_clipped` / `_update_clipped`, arithmetic in csrc/ensemble_clip_body.h): the prepare launch sums the
squares of a model's gradient row in double in a fixed order and writes the scale, the update multiplies the gradient by it.  An
optimizer that was never given one launches the unclipped pair and allocates nothing for it.
"""
import math

import torch

from . import _lib
from .ops import _ld

HYPER = ("lr", "beta1", "beta2", "eps", "weight_decay")   # columns of the hyper table (csrc/ensemble_adam_body.h: EaHyper)
N_COEF = 8                                                 # floats of a model's coefficient row (EaCoef)
_RANGES = {"lr": "lr >= 0", "beta1": "0 <= beta1 < 1", "beta2": "0 <= beta2 < 1", "eps": "eps >= 0", "weight_decay": "weight_decay >= 0"}


def _column(name, value, K):
    """K doubles of one hyper-parameter (a scalar, or one value per model); ValueError outside its range"""
    vals = [float(v) for v in value] if isinstance(value, (list, tuple)) or (torch.is_tensor(value) and value.dim() > 0) else [float(value)] * K
    if len(vals) != K:
        raise ValueError(f"EnsembleAdam: {name} has {len(vals)} values for {K} models")
    for m, v in enumerate(vals):
        if not (0.0 <= v < 1.0 if name.startswith("beta") else 0.0 <= v < float("inf")):
            raise ValueError(f"EnsembleAdam: model {m}: {name} = {v} is outside {_RANGES[name]}")
    return vals


def _max_norms(value, K):
    """K doubles of `max_grad_norm` (a scalar or one entry per model; None or inf: that model is not clipped); ValueError for a
    negative or NaN entry or another length"""
    many = isinstance(value, (list, tuple)) or (torch.is_tensor(value) and value.dim() > 0)
    vals = [math.inf if v is None else float(v) for v in (value if many else [value] * K)]
    if len(vals) != K:
        raise ValueError(f"EnsembleAdam: max_grad_norm has {len(vals)} values for {K} models")
    for m, v in enumerate(vals):
        if not v >= 0.0:
            raise ValueError(f"EnsembleAdam: model {m}: max_grad_norm = {v} is outside max_grad_norm >= 0")
    return vals


class EnsembleAdam:
    def __init__(self, n_models, P, device, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, param_shapes=None, max_grad_norm=None):
        """Every hyper-parameter is a scalar or a length-K sequence.  `param_shapes`: the shapes of one model's parameters in
        `model.parameters()` order, P elements in all (what `state_dict` splits a row by; default: one parameter of P elements).
        `max_grad_norm`: None (no clipping: the unclipped launches), a scalar or a length-K sequence of `clip_grad_norm_`'s
        `max_norm` per model, an entry None or inf meaning that model is not clipped."""
        K, P = int(n_models), int(P)
        if not 1 <= K <= 65535 or P < 1:
            raise ValueError(f"EnsembleAdam: {K} models of {P} parameters (1..65,535 models, at least one parameter)")
        table = [_column("lr", lr, K), _column("beta1", betas[0], K), _column("beta2", betas[1], K), _column("eps", eps, K),
                 _column("weight_decay", weight_decay, K)]
        norms = None if max_grad_norm is None else _max_norms(max_grad_norm, K)   # (refused before anything touches the device)
        self.n_models, self.P, self.device = K, P, torch.device(device)
        self.param_shapes = [torch.Size(s) for s in param_shapes] if param_shapes is not None else [torch.Size((P,))]
        if sum(s.numel() for s in self.param_shapes) != P:
            raise ValueError(f"EnsembleAdam: param_shapes hold {sum(s.numel() for s in self.param_shapes)} elements, not {P}")
        dev = self.device
        self._hyper_host = torch.tensor(table, dtype=torch.float64).t().contiguous()   # [K][5]
        self.hyper = self._hyper_host.to(dev)
        # [K] NicEnsembleAdamState as three doubles a model: the int32 step counter in the first one's low half, c1, c2
        self.state = torch.zeros(K, 3, dtype=torch.float64, device=dev)
        self.state[:, 1:] = 1.0
        self.coef = torch.zeros(K, N_COEF, device=dev)
        self.exp_avg, self.exp_avg_sq = torch.zeros(K, P, device=dev), torch.zeros(K, P, device=dev)
        self.last_kernels = {}
        # clipping: max_norm [K] doubles, clip [K][2] floats {scale, pre-clip norm}; allocated once, when it is first configured
        self.max_norm = self.clip = None
        if norms is not None:
            self._write_max_norms(norms)

    # ---- one step: two launches ------------------------------------------------------------------------------------------------
    def step(self, params, grads, active=None):
        """params [K][>= P] (updated in place), grads [K][>= P]: float32 device tensors with contiguous rows.  `active`: None, or
        an int32 [K] device tensor - a model whose entry is zero sits this step out (`nic_ensemble_adam_prepare_active` /
        `_update_active`: its counter, running products, coef / clip rows, moments and parameters keep their bits)."""
        K, P = self.n_models, self.P
        for name, t in (("params", params), ("grads", grads)):
            if not t.is_cuda:
                raise _lib.NicUnavailableError("EnsembleAdam.step needs device tensors (there is no CPU fallback)")
            if t.dtype != torch.float32 or t.dim() != 2 or t.shape[0] != K or t.shape[1] < P or t.stride(1) != 1:
                raise ValueError(f"EnsembleAdam.step: {name} must be float32 [{K}][>= {P}] with contiguous rows, got {tuple(t.shape)}")
        lib, stream = _lib.lib(), _lib.current_stream()
        if active is not None:
            if not active.is_cuda or active.dtype != torch.int32 or tuple(active.shape) != (K,) or not active.is_contiguous():
                raise ValueError(f"EnsembleAdam.step: active must be a contiguous int32 [{K}] device tensor")
            clipped = self.max_norm is not None
            max_norm, clip = (self.max_norm.data_ptr(), self.clip.data_ptr()) if clipped else (None, None)
            _lib.check(lib.nic_ensemble_adam_prepare_active(K, P, self.hyper.data_ptr(), max_norm, self.state.data_ptr(), self.coef.data_ptr(),
                                                            grads.data_ptr() if clipped else None, _ld(grads) if clipped else 0, clip,
                                                            active.data_ptr(), stream))
            self.last_kernels["prepare"] = lib.nic_last_kernel().decode()
            _lib.check(lib.nic_ensemble_adam_update_active(K, P, params.data_ptr(), _ld(params), grads.data_ptr(), _ld(grads),
                                                           self.exp_avg.data_ptr(), _ld(self.exp_avg), self.exp_avg_sq.data_ptr(),
                                                           _ld(self.exp_avg_sq), self.coef.data_ptr(), clip, active.data_ptr(), stream))
            self.last_kernels["update"] = lib.nic_last_kernel().decode()
            return
        if self.max_norm is not None:
            _lib.check(lib.nic_ensemble_adam_prepare_clipped(K, P, self.hyper.data_ptr(), self.max_norm.data_ptr(), self.state.data_ptr(),
                                                             self.coef.data_ptr(), grads.data_ptr(), _ld(grads), self.clip.data_ptr(), stream))
            self.last_kernels["prepare"] = lib.nic_last_kernel().decode()
            _lib.check(lib.nic_ensemble_adam_update_clipped(K, P, params.data_ptr(), _ld(params), grads.data_ptr(), _ld(grads),
                                                            self.exp_avg.data_ptr(), _ld(self.exp_avg), self.exp_avg_sq.data_ptr(),
                                                            _ld(self.exp_avg_sq), self.coef.data_ptr(), self.clip.data_ptr(), stream))
            self.last_kernels["update"] = lib.nic_last_kernel().decode()
            return
        _lib.check(lib.nic_ensemble_adam_prepare(K, self.hyper.data_ptr(), self.state.data_ptr(), self.coef.data_ptr(), stream))
        self.last_kernels["prepare"] = lib.nic_last_kernel().decode()
        _lib.check(lib.nic_ensemble_adam_update(K, P, params.data_ptr(), _ld(params), grads.data_ptr(), _ld(grads), self.exp_avg.data_ptr(),
                                                _ld(self.exp_avg), self.exp_avg_sq.data_ptr(), _ld(self.exp_avg_sq), self.coef.data_ptr(),
                                                stream))
        self.last_kernels["update"] = lib.nic_last_kernel().decode()

    # ---- hyper-parameters: one device copy, read by the (possibly captured) kernels of the next step ----------------------------
    def _set(self, names, values):
        cols = [_column(n, v, self.n_models) for n, v in zip(names, values)]   # (all checked before anything is written)
        for n, c in zip(names, cols):
            self._hyper_host[:, HYPER.index(n)] = torch.tensor(c, dtype=torch.float64)
        self.hyper.copy_(self._hyper_host)

    def set_lr(self, lrs):
        self._set(["lr"], [lrs])

    def set_betas(self, betas):
        self._set(["beta1", "beta2"], list(betas))

    def set_eps(self, eps):
        self._set(["eps"], [eps])

    def set_weight_decay(self, weight_decay):
        self._set(["weight_decay"], [weight_decay])

    # ---- clipping: one device table too; not Adam state, so no part of `state_dict` ---------------------------------------------------
    def _write_max_norms(self, norms):
        host = torch.tensor(norms, dtype=torch.float64)
        if self.max_norm is None:   # (once: a captured step keeps these addresses)
            self.max_norm = host.to(self.device)
            self.clip = torch.zeros(self.n_models, 2, device=self.device)
            self.clip[:, 0] = 1.0
        else:
            self.max_norm.copy_(host)
        self._max_norm_host = host

    def set_max_grad_norm(self, max_grad_norm):
        """`clip_grad_norm_`'s max_norm from the next step on: a scalar or one entry per model (None or inf: not clipped; None for
        all: every model off).  A replayed clipped step reads the new values; the first configuration of an optimizer built without
        clipping switches it to the clipped launches, which a capture of the unclipped ones does not serve (`capture_key`)."""
        self._write_max_norms(_max_norms(max_grad_norm, self.n_models))

    def max_grad_norm_of(self, m):
        """model m's max norm (host value; inf: not clipped), None for an optimizer without clipping"""
        return None if self.max_norm is None else float(self._max_norm_host[m])

    @property
    def grad_norms(self):
        """[K] device view: every model's total gradient norm of the last step before clipping (what `clip_grad_norm_` returns)"""
        self._require_clipping("grad_norms")
        return self.clip[:, 1]

    @property
    def clip_scales(self):
        """[K] device view: the factor the last step multiplied every model's gradient by (1: not clipped)"""
        self._require_clipping("clip_scales")
        return self.clip[:, 0]

    def _require_clipping(self, what):
        if self.clip is None:
            raise ValueError(f"EnsembleAdam.{what}: this optimizer has no max_grad_norm")

    def capture_key(self):
        """what a captured step bakes in of this optimizer: its buffers' addresses, and with them whether it clips"""
        held = (self.hyper, self.state, self.coef, self.exp_avg, self.exp_avg_sq) + (() if self.max_norm is None else (self.max_norm, self.clip))
        return (self.max_norm is not None,) + tuple(t.data_ptr() for t in held)

    def hyper_of(self, m):
        """{lr, beta1, beta2, eps, weight_decay} of model m (host values)"""
        return dict(zip(HYPER, self._hyper_host[m].tolist()))

    def steps(self):
        """[K] steps taken (reads the device)"""
        return self.state.cpu().view(torch.int32)[:, 0].clone()

    # ---- checkpoints: model m's state as a default torch.optim.Adam over its parameters() saves and loads it ---------------------
    def state_dict(self, m):
        row = self.state[m].cpu()
        step, h = int(row.view(torch.int32)[0]), self.hyper_of(m)
        state, off = {}, 0
        for i, shape in enumerate(self.param_shapes):
            n = shape.numel()
            state[i] = {"step": torch.tensor(float(step), dtype=torch.float32),
                        "exp_avg": self.exp_avg[m, off:off + n].reshape(shape).clone(),
                        "exp_avg_sq": self.exp_avg_sq[m, off:off + n].reshape(shape).clone()}
            off += n
        group = {"lr": h["lr"], "betas": (h["beta1"], h["beta2"]), "eps": h["eps"], "weight_decay": h["weight_decay"], "amsgrad": False,
                 "beta1_power": float(row[1]), "beta2_power": float(row[2]), "params": list(range(len(self.param_shapes)))}
        return {"state": state, "param_groups": [group]}

    def load_state_dict(self, m, sd):
        """The inverse of `state_dict(m)`.  A checkpoint torch wrote has no `beta1_power` / `beta2_power`: they are beta ** step,
        computed on the host."""
        groups = sd["param_groups"]
        if len(groups) != 1 or len(groups[0]["params"]) != len(self.param_shapes):
            raise ValueError("EnsembleAdam.load_state_dict: one parameter group over one model's parameters is expected")
        g = groups[0]
        if g.get("amsgrad") or g.get("maximize"):
            raise ValueError("EnsembleAdam has no amsgrad and no maximize")
        h = [_column(n, v, 1)[0] for n, v in zip(HYPER, (g["lr"], g["betas"][0], g["betas"][1], g["eps"], g["weight_decay"]))]
        entries = [sd["state"].get(k) for k in g["params"]]
        if any(e is None for e in entries) and not all(e is None for e in entries):
            raise ValueError("EnsembleAdam.load_state_dict: some parameters have a state and some have none")
        steps = {int(float(e["step"])) for e in entries if e is not None} or {0}
        if len(steps) != 1:
            raise ValueError(f"EnsembleAdam.load_state_dict: the parameters of one model have different step counts {sorted(steps)}")
        step = steps.pop()
        off = 0
        for e, shape in zip(entries, self.param_shapes):
            n = shape.numel()
            for name, buf in (("exp_avg", self.exp_avg), ("exp_avg_sq", self.exp_avg_sq)):
                if e is None:
                    buf[m, off:off + n] = 0.0
                else:
                    if tuple(e[name].shape) != tuple(shape):
                        raise ValueError(f"EnsembleAdam.load_state_dict: {name} of shape {tuple(e[name].shape)} for a parameter of {tuple(shape)}")
                    buf[m, off:off + n].copy_(e[name].reshape(-1))
            off += n
        row = torch.zeros(3, dtype=torch.float64)
        row.view(torch.int32)[0] = step
        row[1] = float(g["beta1_power"]) if "beta1_power" in g else h[1] ** step
        row[2] = float(g["beta2_power"]) if "beta2_power" in g else h[2] ** step
        self.state[m].copy_(row)
        self._hyper_host[m] = torch.tensor(h, dtype=torch.float64)
        self.hyper.copy_(self._hyper_host)
