"""What the K-model engines (`SmallPolicyEnsemble`, `HorizonPolicyEnsemble`) share around their `train_step`: binding the models'
parameters to the rows of `weights [K][P]`, the optimizer check, and the epoch loop `fit` / `load_best` with the best weights per
model kept on the device.  An engine provides `n_models`, `device`, `problem_params`, `weights`, `_bind_requested`, `_bound`,
`best_dev`, `best_weights`, `train_step` and `run`."""
import torch

from .ensemble_adam import EnsembleAdam


def bind_rows(linears_per_model, weights, slices):
    """weight.data / bias.data of every layer <- views of the model's row of `weights`; slices: [(weight offset, rows, cols, bias
    offset)] per layer.  The rows must already hold the current values."""
    for m, ls in enumerate(linears_per_model):
        row = weights[m]
        for lin, (o, n, k, bo) in zip(ls, slices):
            lin.weight.data = row[o:o + n * k].view(n, k)
            lin.bias.data = row[bo:bo + n]


def materialized_width(models):
    """the first layer's input width if some model's first layer is materialised (not a LazyLinear any more), else None"""
    known = [ls[0].in_features for ls in (m.master_linears() for m in models)
             if not isinstance(ls[0].weight, torch.nn.parameter.UninitializedParameter)]
    return known[0] if known else None


class EnsembleStep:
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

    # ---- epochs ------------------------------------------------------------------------------------------------------------------
    def fit(self, train_batches, dev_batches, epochs, periods, dev_periods, ignore_periods, optimizer, observation_params=None):
        """`epochs` times: `train_step` over `train_batches`, then `run(train=False)` over `dev_batches` (each batch a dict, or -
        where the engine takes them - a list of I instances' dicts; the sample count is per instance).  Returns the train and dev
        histories [epochs][K]: the reported cost per (scenario, reported period, store) as `Trainer.do_one_epoch` averages it.
        The best dev loss per model and the parameters that gave it are tracked on the device (`best_dev [K]`, `best_weights
        [K][P]`, updated with a mask): no host synchronisation inside an epoch.  `load_best()` puts them back."""
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

    def load_best(self):
        """bound parameters <- `best_weights` (the parameters after the epoch with each model's lowest dev loss)"""
        if self.best_weights is None or not self._bound:
            raise ValueError(f"{type(self).__name__}.load_best: no fit() has run on bound parameters")
        self.weights.copy_(self.best_weights)
