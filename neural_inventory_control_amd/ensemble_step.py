"""What the K-model engines (`SmallPolicyEnsemble`, `HorizonPolicyEnsemble`) share around their kernels.

The packed-row layout: `weights [K][P]`, row m = model m's layers in `nn.Linear`'s own order (per layer the weight, row-major, then
the bias) - `layer_slices`, `packed_count`, `grad_views`, `pack_ensemble_weights`, all on `dims = [F, H1, ..., n_out]`.

`EnsembleStep`, the engines' base: the one problem cache of the ensemble, materialising (policy_layers.py, in model order) and
comparing the models' layers, `weights` and binding the models' parameters to its rows, what a step does with the
weights before it launches (bound: nothing; bind requested: bind on the first batch; else pack, every run), the frames of `run` and
`train_step` around an engine's `_step`, the active-model mask (`active`, `set_active`: int32 [K] on the device, read by the launches
that take one: all of `SmallPolicyEnsemble`'s; `HorizonPolicyEnsemble`'s optimizer, and all of its launches with `skip_inactive`,
which `fit(trainer_params=...)` switches on for its duration), and the epoch loop `fit` / `load_best` with the best weights per model kept on the device - with `trainer_params`,
`Trainer.train`'s dev schedule, best-model choice and early stopping per model (`early_stopping_update`, a pure function).
An engine provides `_step`, `run` and `train_step` with its own signatures, and sizes `grad` / `_grad_views` with its buffers.
`check_model_list` is the part of the engines' `check_models` that does not depend on the policy."""
import copy

import torch

from . import _lib
from . import small_rollout as sr
from .ensemble_adam import EnsembleAdam
from .layout import EnvProblem, ProblemCache, Table
from .policy_layers import materialize_linears, materialized_linears, supports

MAX_MODELS = 65535   # (grid y = model)


def layer_slices(dims):
    """[(weight offset, rows, cols, bias offset)] per layer of one model's packed row; dims = [F, H1, ..., n_out]"""
    out, off = [], 0
    for k, n in zip(dims[:-1], dims[1:]):
        out.append((off, n, k, off + n * k))
        off += n * k + n
    return out


def packed_count(dims):
    return sum(n * k + n for k, n in zip(dims[:-1], dims[1:]))


def grad_views(grad, dims):
    """[(weight gradients per layer, bias gradients per layer)] per model: views into grad [K][>= P] in the packed-weight layout"""
    sl = layer_slices(dims)
    return [([grad[m, o:o + n * k].view(n, k) for o, n, k, _ in sl], [grad[m, bo:bo + n] for _, n, _, bo in sl])
            for m in range(grad.shape[0])]


def pack_ensemble_weights(linears_per_model, out=None):
    """[K][P]: row m = `pack_weights` of model m's layers, all K models in ONE torch.cat (one launch)."""
    K = len(linears_per_model)
    flat = sr.pack_weights([lin for lins in linears_per_model for lin in lins], None if out is None else out.view(-1))
    if flat.numel() % K != 0:
        raise ValueError("pack_ensemble_weights: the models do not have the same number of parameters")
    return flat.view(K, -1) if out is None else out


def materialized_width(models):
    """the first layer's input width if some model's first layer is materialised (not a LazyLinear any more), else None"""
    known = [ls[0].in_features for ls in (m.master_linears() for m in models)
             if not isinstance(ls[0].weight, torch.nn.parameter.UninitializedParameter)]
    return known[0] if known else None


def check_model_list(models, who, policies, handles, arch, mismatch, own=None, versus_first=None):
    """What engine `who` asks of its models whatever the policy: 1..65,535 of them, each a policy named in `policies` that
    `FusedRollout` takes (else "`who` handles `handles`"), with a bias in every layer and `arch(model)` equal to model 0's
    (`mismatch`: the message's format for the two).  The engine's own rules keep their places: `own(i, model)`, on one model,
    follows the policy check; `versus_first(i, model, first)` follows the architecture's.  ValueError names the first mismatch.
    Host-side only."""
    models = list(models)
    if len(models) < 1:
        raise ValueError(f"{who} needs at least one model")
    if len(models) > MAX_MODELS:
        raise ValueError(f"{who} takes at most 65,535 models")
    for i, m in enumerate(models):
        name = getattr(m, "nn_args", {}).get("name") if hasattr(m, "nn_args") else None
        if name not in policies or not supports(m):
            raise ValueError(f"model {i}: {who} handles {handles}, got {name!r}")
        if own is not None:
            own(i, m)
        if any(lin.bias is None for lin in m.master_linears()):
            raise ValueError(f"model {i}: a layer without bias")
        if arch(m) != arch(models[0]):
            raise ValueError(f"model {i}: " + mismatch.format(arch(m), arch(models[0])))
        if versus_first is not None:
            versus_first(i, m, models[0])
    return models


# ---- I problem instances under one launch pair (the engines stage a list of batches with these) -------------------------------------
def instance_replicas(n_instances, n_models, who):
    """models per problem instance; the instances must divide the K models (needs the batches' count only: the engines ask before
    anything is built from the batches)"""
    if n_instances < 1 or n_models % n_instances != 0:
        raise ValueError(f"{who}: {n_instances} problem instances do not divide {n_models} models")
    return n_models // n_instances


def check_instances(probs, n_models, trace_lengths=None, who="SmallPolicyEnsemble"):
    """The problem instances one launch pair takes: I >= 1 `EnvProblem`s, I dividing the K models, that agree in everything the
    kernels take once - B, the pipeline shape, the flags, the trace length (`trace_lengths`, one per instance, if given) and every
    table's layout (present or not, uniform or per-scenario: one descriptor addresses all instances).  ValueError names the first
    mismatch; `who`: the engine the messages name.  Host-side only.  Returns the replicas per instance."""
    probs = list(probs)
    if len(probs) < 1:
        raise ValueError(f"{who} needs at least one problem instance")
    replicas = instance_replicas(len(probs), n_models, who)
    first = probs[0]
    for i, p in enumerate(probs[1:], 1):
        if p.B != first.B:
            raise ValueError(f"instance {i}: {p.B} scenarios, instance 0 has {first.B}")
        if trace_lengths is not None and trace_lengths[i] != trace_lengths[0]:
            raise ValueError(f"instance {i}: a demand trace of {trace_lengths[i]} periods, instance 0's has {trace_lengths[0]}")
        shape = lambda q: (q.S, q.Wn, q.E, q.Ws, q.Ww, q.We)  # noqa: E731
        if shape(p) != shape(first):
            raise ValueError(f"instance {i}: pipeline shape (S, Wn, E, Ws, Ww, We) = {shape(p)} differs from instance 0's {shape(first)}")
        if (p.lost_demand, p.maximize_profit) != (first.lost_demand, first.maximize_profit):
            raise ValueError(f"instance {i}: lost_demand / maximize_profit differ from instance 0's")
        for name in EnvProblem._TABLES:
            a, b = getattr(first, name), getattr(p, name)
            if (a.tensor is None) != (b.tensor is None):
                raise ValueError(f"instance {i}: table {name!r} is {'missing' if b.tensor is None else 'present'}, instance 0's is not")
            if a.tensor is not None and (a.scn_stride == 0) != (b.scn_stride == 0):
                kind = lambda t: "uniform" if t.scn_stride == 0 else "per-scenario"  # noqa: E731
                raise ValueError(f"instance {i}: table {name!r} is {kind(b)}, instance 0's is {kind(a)}")
            if a.tensor is not None and ((tuple(a.tensor.shape), a.loc_stride, a.sup_stride)
                                         != (tuple(b.tensor.shape), b.loc_stride, b.sup_stride)):
                raise ValueError(f"instance {i}: table {name!r} has shape {tuple(b.tensor.shape)}, instance 0's {tuple(a.tensor.shape)}")
    return replicas


def stack_instance_tables(probs):
    """An `EnvProblem` like probs[0] whose tables are [I][...] stacks of the instances' (instance 0 first: a descriptor built from it
    points at instance 0, instance i's copy of a table starts i x the returned stride behind) and {table: stride in floats}."""
    stacked, strides = copy.copy(probs[0]), {}
    for name in EnvProblem._TABLES:
        t = getattr(probs[0], name)
        if t.tensor is None:
            continue
        tensor = torch.stack([getattr(p, name).tensor.contiguous() for p in probs])
        setattr(stacked, name, Table(tensor, t.loc_stride, t.scn_stride, t.sup_stride))
        strides[name] = tensor[0].numel()
    return stacked, strides


def refresh_instance_tables(stacked, sources, probs):
    """The instances' tables into `stacked`'s (what `stack_instance_tables` made of `sources`), in place, if `probs` are other
    batches' problems than `sources` (the problem cache hands the same object out for the same tensors).  Returns the sources now."""
    if all(a is b for a, b in zip(sources, probs)):
        return sources
    for name in EnvProblem._TABLES:
        tensor = getattr(stacked, name).tensor
        if tensor is not None:
            for i, p in enumerate(probs):
                tensor[i].copy_(getattr(p, name).tensor)
    return probs


def table_layouts(prob):
    """what a list-of-instances batch adds to a batch shape's key for its tables: (table, scenario stride) of those present"""
    return tuple((name, getattr(prob, name).scn_stride) for name in EnvProblem._TABLES if getattr(prob, name).tensor is not None)


# ---- per-model early stopping: Trainer.train's bookkeeping (trainer.py:182-194, :547-556) on [K] tensors ------------------------------
BEST_MODEL_CHOICES = ("dev_loss", "train_loss")


def read_trainer_params(trainer_params):
    """(do_dev_every_n_epochs, choose_best_model_on, early_stopping_patience_epochs or None) of a `trainer_params` dict; ValueError
    for a value `Trainer.train` could not run with"""
    every, choose = int(trainer_params["do_dev_every_n_epochs"]), trainer_params["choose_best_model_on"]
    patience = trainer_params.get("early_stopping_patience_epochs", None)
    if every < 1:
        raise ValueError(f"do_dev_every_n_epochs must be at least 1, got {every}")
    if choose not in BEST_MODEL_CHOICES:
        raise ValueError(f"choose_best_model_on is one of {BEST_MODEL_CHOICES}, got {choose!r}")
    if patience is not None and int(patience) < 0:
        raise ValueError(f"early_stopping_patience_epochs must be None or at least 0, got {patience}")
    return every, choose, None if patience is None else int(patience)


def early_stopping_update(train_loss, dev_loss, best_train, best_dev, best_epoch, active, epoch, trainer_params):
    """What `Trainer.train` does after a dev evaluation (`update_best_params_and_save`, then the patience test), for K models at
    once: model m is better if its chosen loss (`choose_best_model_on`) is strictly below its best; a better model's best train and
    dev loss and best epoch become this epoch's; a model stops when `epoch - best_epoch >= early_stopping_patience_epochs` (absent
    or None: never).  Models that are not `active` change nothing.  All [K] tensors (`best_epoch` int64, `active` bool) on any
    device, `epoch` an int; nothing is modified in place and nothing is read back.
    Returns (better, best_train, best_dev, best_epoch, active): `better` is the mask the caller copies the weights under."""
    _, choose, patience = read_trainer_params(trainer_params)
    current, best = (dev_loss, best_dev) if choose == "dev_loss" else (train_loss, best_train)
    better = (current < best) & active
    best_train = torch.where(better, train_loss, best_train)
    best_dev = torch.where(better, dev_loss, best_dev)
    best_epoch = torch.where(better, torch.full_like(best_epoch, epoch), best_epoch)
    if patience is not None:
        active = active & ~((epoch - best_epoch) >= patience)
    return better, best_train, best_dev, best_epoch, active


class EnsembleStep:
    def __init__(self, models, problem_params, device):
        """`models`: what the engine's `check_models` returned"""
        _lib.require_device()
        self.models, self.problem_params, self.device = models, problem_params, torch.device(device)
        self._problems = ProblemCache()   # (one for the ensemble: the same tensors presented again give the same `EnvProblem` object)
        self.last_kernels = {}          # launch class -> kernel name the library recorded in the last run
        self.weights = self.grad = self._grad_views = None   # [K][P], [K][>= P]: once per engine
        self.param_shapes = None        # shapes of one model's parameters in `parameters()` order (EnsembleAdam's `param_shapes`)
        self._bind_requested = self._bound = False
        self._dims_bound = None         # layer sizes, once the parameters are bound
        self.best_dev = self.best_weights = None   # `fit`: [K] lowest dev loss so far, [K][P] the parameters that gave it
        # `fit(trainer_params=...)`: [K] the train loss that went with the best, the epoch of the best, the epoch a model stopped at (-1: never)
        self.best_train = self.best_epoch = self.stopped_epoch = None
        # the active-model mask: allocated once (a captured step keeps its address and reads its current contents); not in use -
        # nothing launches with it - until `set_active` is given one
        self.active = torch.ones(len(models), dtype=torch.int32, device=self.device)
        self._masked = False

    @property
    def n_models(self):
        return len(self.models)

    # ---- the active-model mask ----------------------------------------------------------------------------------------------------------
    def set_active(self, mask):
        """Which models the next runs and steps take: a length-K sequence or tensor, non-zero / True = the model runs (written into
        `active` in place - a replayed capture follows it); None: every model, through the launches without a mask again.  An
        inactive model's weights row, optimizer state and buffers keep their bits, and its entries of the returned totals are NaN."""
        if mask is None:
            self.active.fill_(1)
            self._masked = False
            return
        mask = torch.as_tensor(mask)
        if tuple(mask.shape) != (self.n_models,):
            raise ValueError(f"{type(self).__name__}.set_active: a mask of {self.n_models} entries is expected, got {tuple(mask.shape)}")
        self.active.copy_((mask != 0).to(device=self.device, dtype=torch.int32))
        self._masked = True

    def active_models(self):
        """bool [K] on the host: the models the next run takes (reads the device)"""
        return self.active.cpu() != 0

    def _mask(self):
        """what the launches get as `active`: the mask once one has been set, else None (the launches as they always were)"""
        return self.active if self._masked else None

    def _mask_totals(self, tt):
        """NaN into the rows of a run's totals [K][2] that belong to inactive models (their launches wrote nothing there)"""
        return tt if not self._masked else torch.where((self.active != 0)[:, None], tt, torch.full_like(tt, float("nan")))

    def _note(self, tag):
        name = _lib.lib().nic_last_kernel()
        self.last_kernels[tag] = name.decode() if name else None

    # ---- the models' layers and the rows of `weights` -------------------------------------------------------------------------------------
    def _materialize(self, F):
        """(every model's layers, their common sizes [F, H1, ..., n_out]), LazyLinear first layers materialised for F inputs"""
        for m in self.models:
            materialize_linears(m.master_linears(), F)
        lins = self._linears()
        dims = [[ls[0].in_features] + [m.out_features for m in ls] for ls in lins]
        for i, d in enumerate(dims):
            if d != dims[0]:
                raise ValueError(f"model {i}: layer sizes {d} differ from model 0's {dims[0]}")
        return lins, dims[0]

    def _linears(self):
        """every model's materialised layers"""
        return [materialized_linears(m) for m in self.models]

    def _problem_for(self, data):
        """EnvProblem of a batch (cached per presented tensors, see layout.ProblemCache)"""
        return self._problems.get(self.problem_params, data, self.device)

    def _layers(self, F):
        """(layers, sizes) a step on F input rows runs with; bound: (None, the bound sizes) - nothing is packed, and the per-model
        checks were made when the parameters were bound"""
        return (None, self._dims_bound) if self._bound else self._materialize(F)

    def _model_buffers(self, dims):
        """`weights [K][P]` for these layer sizes.  Other sizes than before (a LazyLinear model materialised anew) allocate again,
        and the gradient buffer goes with them; bound parameters cannot change theirs."""
        P = packed_count(dims)
        if self.weights is None or self.weights.shape[1] != P:
            if self._bound:
                raise ValueError(f"{type(self).__name__}: layer sizes {list(dims)} differ from the bound parameters'")
            self.weights, self.grad, self._grad_views = torch.zeros(self.n_models, P, device=self.device), None, None
            self.param_shapes = [shape for _, n, k, _ in layer_slices(dims) for shape in ((n, k), (n,))]

    def _bind(self, lins, dims):
        """weight.data / bias.data of every layer <- views of the model's row of `weights`, which gets the current values once"""
        pack_ensemble_weights(lins, self.weights)
        for m, ls in enumerate(lins):
            row = self.weights[m]
            for lin, (o, n, k, bo) in zip(ls, layer_slices(dims)):
                lin.weight.data = row[o:o + n * k].view(n, k)
                lin.bias.data = row[bo:bo + n]
        self._bound, self._dims_bound = True, list(dims)

    def bind_parameters(self):
        """Opt-in: from now on the models' parameters LIVE in `weights [K][P]` (views of their rows), `run` and `train_step` pack
        nothing, and whatever writes a parameter in place - `load_state_dict`, an optimizer - writes the packed row.  Binds now if
        the input width is known (a materialised first layer), else on the first batch."""
        self._bind_requested = True
        F = materialized_width(self.models)
        if F is not None and not self._bound:
            lins, dims = self._materialize(F)
            self._model_buffers(dims)
            self._bind(lins, dims)

    def _ready_weights(self, lins, dims, optimizer):
        """A step, once the engine's `_setup` sized `weights` and before anything is launched: the optimizer must be one for (K, P);
        then `weights` gets the parameters - bound, they live there; bind requested, they do from this first batch on; else they
        are packed, every run (the caller's optimizers moved them)."""
        if optimizer is not None:
            self._require_optimizer_shape(optimizer)
        if self._bound:
            return
        if self._bind_requested:
            self._bind(lins, dims)
        else:
            pack_ensemble_weights(lins, self.weights)

    def param_grads(self):
        """[(parameter, gradient view into the [K][P] buffer of the last training run)] over all models"""
        out = []
        for lins, (gw, gb) in zip(self._linears(), self._grad_views):
            for i, m in enumerate(lins):
                out += [(m.weight, gw[i]), (m.bias, gb[i])]
        return out

    # ---- the frames of `run` and `train_step`; `batch`: the engine's `_step` arguments before train, discrete_allocation, optimizer -----
    def _run(self, batch, train, accumulate_grads, discrete_allocation):
        if discrete_allocation and train:
            raise ValueError("discrete_allocation is an evaluation-time option of the fused rollout")
        tt = self._step(*batch, train=train, discrete_allocation=discrete_allocation, optimizer=None)
        if train:
            sr.assign_grads(self.param_grads(), accumulate_grads)
        return tt[:, 0], tt[:, 1]

    def _train_step(self, batch, optimizer):
        self._require_step(optimizer)
        tt = self._step(*batch, train=True, discrete_allocation=False, optimizer=optimizer)
        return tt[:, 0], tt[:, 1]

    def _require_step(self, optimizer):
        """`train_step`'s preconditions that need no device: bound parameters, an EnsembleAdam"""
        who = type(self).__name__
        if not self._bind_requested:
            raise ValueError(f"{who}.train_step needs bound parameters: call bind_parameters() first")
        if not isinstance(optimizer, EnsembleAdam):
            raise ValueError(f"{who}.train_step needs an EnsembleAdam as `optimizer`")

    def _require_optimizer_shape(self, optimizer):
        if (optimizer.n_models, optimizer.P) != tuple(self.weights.shape):
            raise ValueError(f"{type(self).__name__}.train_step: the optimizer is for {optimizer.n_models} models of {optimizer.P} "
                             f"parameters, the engine has {self.weights.shape[0]} of {self.weights.shape[1]}")

    def make_optimizer(self, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, max_grad_norm="models"):
        """An `EnsembleAdam` for this engine's (K, P) and parameter shapes.  `max_grad_norm`: "models" clips model m's gradient norm at
        its `gradient_clipping_norm_value` as the trainer does (trainer.py:175-176; None there: that model is not clipped, and with
        no model that has one the optimizer is an unclipped one); else what `EnsembleAdam` takes.  Needs sized weights: bound
        parameters or a first batch."""
        if self.weights is None:
            raise ValueError(f"{type(self).__name__}.make_optimizer needs sized weights: bind_parameters() on materialised models, or a "
                             "first batch")
        if isinstance(max_grad_norm, str):
            if max_grad_norm != "models":
                raise ValueError(f"{type(self).__name__}.make_optimizer: max_grad_norm is \"models\", None, a number or one per model")
            max_grad_norm = [getattr(m, "gradient_clipping_norm_value", None) for m in self.models]
            if all(v is None for v in max_grad_norm):
                max_grad_norm = None
        K, P = self.weights.shape
        return EnsembleAdam(K, P, self.device, lr, betas=betas, eps=eps, weight_decay=weight_decay, param_shapes=self.param_shapes,
                            max_grad_norm=max_grad_norm)

    # ---- epochs ------------------------------------------------------------------------------------------------------------------
    def fit(self, train_batches, dev_batches, epochs, periods, dev_periods, ignore_periods, optimizer, observation_params=None,
            trainer_params=None):
        """`epochs` times: `train_step` over `train_batches`, then `run(train=False)` over `dev_batches` (each batch a dict, or -
        where the engine takes them - a list of I instances' dicts; the sample count is per instance).  Returns the train and dev
        histories [epochs][K]: the reported cost per (scenario, reported period, store) as `Trainer.do_one_epoch` averages it.
        The best dev loss per model and the parameters that gave it are tracked on the device (`best_dev [K]`, `best_weights
        [K][P]`, updated with a mask): no host synchronisation inside an epoch.  `load_best()` puts them back.
        `trainer_params` (a dict with `do_dev_every_n_epochs`, `choose_best_model_on`, optionally `early_stopping_patience_epochs`):
        `Trainer.train`'s protocol per model instead - see `_fit_protocol`."""
        if trainer_params is not None:
            return self._fit_protocol(train_batches, dev_batches, epochs, periods, dev_periods, ignore_periods, optimizer,
                                      observation_params, trainer_params)
        K, dev = self.n_models, self.device
        hist = [torch.zeros(epochs, K, device=dev), torch.zeros(epochs, K, device=dev)]
        n_stores = self.problem_params["n_stores"]
        for epoch in range(epochs):
            for which, batches, T in ((0, train_batches, periods), (1, dev_batches, dev_periods)):
                samples = 0
                for data in batches:
                    if which == 0:
                        _, reported = self.train_step(data, T, ignore_periods, optimizer, observation_params)
                    else:
                        _, reported = self.run(data, T, ignore_periods, train=False, observation_params=observation_params)
                    hist[which][epoch] += reported
                    samples += (data[0] if isinstance(data, (list, tuple)) else data)["demands"].shape[0]   # (per instance)
                if samples == 0:
                    raise ValueError(f"{type(self).__name__}.fit needs at least one training batch and one dev batch")
                hist[which][epoch] /= float(samples * (T - ignore_periods) * n_stores)
            if self.best_dev is None:
                self.best_dev = torch.full((K,), float("inf"), device=dev)
                self.best_weights = self.weights.clone()
            better = hist[1][epoch] < self.best_dev
            self.best_dev = torch.where(better, hist[1][epoch], self.best_dev)
            self.best_weights = torch.where(better[:, None], self.weights, self.best_weights)
        return hist[0], hist[1]

    def _epoch_loss(self, batches, T, ignore_periods, optimizer, observation_params):
        """[K] reported cost per (scenario, reported period, store) of one pass over `batches`; `optimizer`: a training pass"""
        total, samples = torch.zeros(self.n_models, device=self.device), 0
        for data in batches:
            if optimizer is not None:
                _, reported = self.train_step(data, T, ignore_periods, optimizer, observation_params)
            else:
                _, reported = self.run(data, T, ignore_periods, train=False, observation_params=observation_params)
            total += reported
            samples += (data[0] if isinstance(data, (list, tuple)) else data)["demands"].shape[0]   # (per instance)
        if samples == 0:
            raise ValueError(f"{type(self).__name__}.fit needs at least one training batch and one dev batch")
        return total / float(samples * (T - ignore_periods) * self.problem_params["n_stores"])

    def _fit_protocol(self, train_batches, dev_batches, epochs, periods, dev_periods, ignore_periods, optimizer, observation_params,
                      trainer_params):
        """`fit` as `Trainer.train` runs it (trainer.py:177-197), per model: the dev set is evaluated when `epoch %
        do_dev_every_n_epochs == 0` (else the dev history repeats its last entry); after it, a model whose `choose_best_model_on`
        loss is strictly below its best gets new `best_train`, `best_dev`, `best_epoch` and `best_weights` row, and a model with
        `epoch - best_epoch >= early_stopping_patience_epochs` stops: from the next epoch on it is not in `active`, so the launches
        that read the mask skip it and the optimizer leaves its row alone.  Starts with every model active and leaves the mask as
        it ends.  Returns the histories [epochs][K], NaN for a model after its stop (and for every model once all have stopped and
        the loop ended); `stopped_epoch [K]`: the epoch of the stop, -1 for none.
        All of it is [K]-sized work on the device, nothing per batch; the one host read is per dev evaluation (only with a
        patience), to end the loop when no model is left.  No checkpoints are written (`save_model`, `epochs_between_save`)."""
        every, _, patience = read_trainer_params(trainer_params)
        if hasattr(self, "skip_inactive"):   # an engine whose launches skip the stopped models on request only: for this fit, they do
            previous, self.skip_inactive = self.skip_inactive, True
            try:
                return self._protocol_epochs(train_batches, dev_batches, epochs, periods, dev_periods, ignore_periods, optimizer,
                                             observation_params, trainer_params, every, patience)
            finally:
                self.skip_inactive = previous
        return self._protocol_epochs(train_batches, dev_batches, epochs, periods, dev_periods, ignore_periods, optimizer,
                                     observation_params, trainer_params, every, patience)

    def _protocol_epochs(self, train_batches, dev_batches, epochs, periods, dev_periods, ignore_periods, optimizer, observation_params,
                         trainer_params, every, patience):
        """the epochs of `_fit_protocol`"""
        K, dev = self.n_models, self.device
        nan = torch.full((K,), float("nan"), device=dev)
        hist = [torch.full((epochs, K), float("nan"), device=dev), torch.full((epochs, K), float("nan"), device=dev)]
        self.set_active(torch.ones(K))
        active = torch.ones(K, dtype=torch.bool, device=dev)
        self.best_epoch = torch.zeros(K, dtype=torch.int64, device=dev)          # (Trainer.best_epoch starts at 0)
        self.stopped_epoch = torch.full((K,), -1, dtype=torch.int64, device=dev)
        for epoch in range(epochs):
            # (launches that do not read the mask still compute a stopped model's costs: they do not surface)
            hist[0][epoch] = torch.where(active, self._epoch_loss(train_batches, periods, ignore_periods, optimizer, observation_params), nan)
            if epoch % every != 0:
                hist[1][epoch] = torch.where(active, hist[1][epoch - 1], nan)
                continue
            hist[1][epoch] = torch.where(active, self._epoch_loss(dev_batches, dev_periods, ignore_periods, None, observation_params), nan)
            if self.best_dev is None:
                self.best_dev = torch.full((K,), float("inf"), device=dev)
                self.best_weights = self.weights.clone()
            if self.best_train is None:
                self.best_train = torch.full((K,), float("inf"), device=dev)
            better, self.best_train, self.best_dev, self.best_epoch, still = early_stopping_update(
                hist[0][epoch], hist[1][epoch], self.best_train, self.best_dev, self.best_epoch, active, epoch, trainer_params)
            self.best_weights = torch.where(better[:, None], self.weights, self.best_weights)
            self.stopped_epoch = torch.where(active & ~still, torch.full_like(self.stopped_epoch, epoch), self.stopped_epoch)
            active = still
            self.active.copy_(active.to(torch.int32))
            if patience is not None and not bool(active.any()):   # (the one host read)
                break
        return hist[0], hist[1]

    def load_best(self):
        """bound parameters <- `best_weights` (the parameters after the epoch with each model's lowest dev loss)"""
        if self.best_weights is None or not self._bound:
            raise ValueError(f"{type(self).__name__}.load_best: no fit() has run on bound parameters")
        self.weights.copy_(self.best_weights)
