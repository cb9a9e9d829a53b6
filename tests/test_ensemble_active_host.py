"""Host side of per-model early stopping in the K-model sweeps (the `_active` entry points, `EnsembleStep.fit(trainer_params=...)`):
the request checks of the active-model mask through a stand-alone program built with the host compiler, the per-model protocol
function against a literal transcription of `Trainer.train` / `update_best_params_and_save`, and the C declarations against their
ctypes prototypes."""
import itertools
import math
import os
import re
import subprocess

import pytest
import torch

from neural_inventory_control_amd import _lib, ensemble_step as es
from test_small_ensemble_host import _host_clang

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SE_OK, SE_ACTIVE = 0, 13
EA_OK, EA_MODELS, EA_COLUMNS, EA_NULL, EA_PARAMS, EA_GRADS, EA_EXP_AVG, EA_EXP_AVG_SQ, EA_ACTIVE, EA_TOGETHER = range(10)
MASK_REASON = "the active mask must be NULL or 4-byte aligned"


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("ensemble_active") / "harness")
    # (-Wall -Werror: the headers have to stay clean C++ for a compiler that knows nothing of HIP)
    subprocess.run([_host_clang(), "-O1", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-o", exe,
                    os.path.join(ROOT, "tests", "ensemble_active_harness.cpp")], check=True)

    def run(*args):
        return subprocess.run([exe] + [a if isinstance(a, str) else str(int(a)) for a in args], check=True, capture_output=True,
                              text=True).stdout.strip()
    return run


# ---- the request checks ---------------------------------------------------------------------------------------------------------------
def test_rollout_mask_check_accepts_null_and_aligned_and_names_the_refusal(harness):
    assert harness("rollout", 0) == "0 accepted"            # NULL: every model runs
    assert harness("rollout", 0x7000) == harness("rollout", 0x7004) == "0 accepted"
    for off in (1, 2, 3):
        assert harness("rollout", 0x7000 + off) == f"{SE_ACTIVE} {MASK_REASON}"


def test_adam_prepare_check_accepts_both_steps_and_names_every_refusal(harness):
    A = 0x1000   # (any aligned non-null address: nothing is dereferenced)

    def prepare(n_models=3, P=10, hyper=A, max_norm=A, state=A, coef=A, grads=A, grads_stride=12, clip=A, active=A):
        code, reason = harness("prepare", n_models, P, hyper, max_norm, state, coef, grads, grads_stride, clip, active).split(" ", 1)
        return int(code), reason

    assert prepare() == (EA_OK, "accepted") and prepare(active=0) == (EA_OK, "accepted")                       # clipped, with / without mask
    unclipped = dict(max_norm=0, clip=0, grads=0, grads_stride=0, P=0)
    assert prepare(**unclipped)[0] == EA_OK and prepare(active=0, **unclipped)[0] == EA_OK                     # (P is not read then)
    assert prepare(n_models=65535)[0] == EA_OK
    assert prepare(n_models=0)[0] == prepare(n_models=65536)[0] == EA_MODELS
    for name in ("hyper", "state", "coef"):
        assert prepare(**{name: 0})[0] == EA_NULL, name
    for kw in (dict(max_norm=0), dict(clip=0), dict(grads=0), dict(max_norm=0, clip=0), dict(max_norm=0, grads=0), dict(clip=0, grads=0)):
        assert prepare(**kw) == (EA_TOGETHER, "max_norm, clip and the gradients go together"), kw
    assert prepare(P=0)[0] == EA_COLUMNS
    assert prepare(grads_stride=9)[0] == EA_GRADS
    for off in (1, 2, 3):
        assert prepare(active=A + off) == (EA_ACTIVE, MASK_REASON)
        assert prepare(active=A + off, **unclipped)[0] == EA_ACTIVE


def test_adam_update_check_accepts_both_steps_and_names_every_refusal(harness):
    A = 0x1000

    def update(n_models=3, P=10, params=A, ps=10, grads=A, gs=12, exp_avg=A, es_=10, exp_avg_sq=A, ess=11, coef=A, active=A):
        return int(harness("update", n_models, P, params, ps, grads, gs, exp_avg, es_, exp_avg_sq, ess, coef, active).split()[0])

    assert update() == EA_OK and update(active=0) == EA_OK
    assert update(n_models=0) == update(n_models=65536) == EA_MODELS
    assert update(P=0) == EA_COLUMNS
    for name in ("params", "grads", "exp_avg", "exp_avg_sq", "coef"):
        assert update(**{name: 0}) == EA_NULL, name
    assert (update(ps=9), update(gs=9), update(es_=9), update(ess=9)) == (EA_PARAMS, EA_GRADS, EA_EXP_AVG, EA_EXP_AVG_SQ)
    assert [update(active=A + off) for off in (1, 2, 3)] == [EA_ACTIVE] * 3


def test_the_kernels_predicates_and_the_recorded_names(harness):
    mask = [1, 0, 1, 0, 0, 7, -1]
    flags = harness("runs", *mask).split()
    assert flags[:len(mask)] == ["11" if v else "00" for v in mask]        # non-zero: the model runs, in both predicates
    assert flags[len(mask):] == ["11"] * len(mask)                         # NULL: every model runs
    assert harness("name", 0, 16, 3, 1, 8, 0, 1) == "small_rollout16_fwd_kernel<3,one_store,models=8,active>"
    assert harness("name", 1, 32, 2, 2, 4, 2, 1) == "small_rollout_bwd_mfma_kernel<2,wgrad,serial,models=4,instances=2,active>"
    assert harness("name", 1, 32, 2, 2, 4, 2, 0) == "small_rollout_bwd_mfma_kernel<2,wgrad,serial,models=4,instances=2>"   # (as it was)


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------
ENTRY_POINTS = {"nic_small_rollout_ensemble_fwd_active": 9, "nic_small_rollout_ensemble_bwd_wgrad_active": 10,
                "nic_small_rollout_ensemble_reduce_active": 13, "nic_small_rollout_instances_fwd_active": 10,
                "nic_small_rollout_instances_bwd_wgrad_active": 11, "nic_ensemble_adam_prepare_active": 11,
                "nic_ensemble_adam_update_active": 14}
C_TYPES = {"const NicSmallRolloutDesc*": "LP_NicSmallRolloutDesc", "const NicSmallEnsemble*": "LP_NicSmallEnsemble",
           "const NicSmallInstances*": "LP_NicSmallInstances", "float*": "c_void_p", "const float*": "c_void_p", "void*": "c_void_p",
           "const double*": "c_void_p", "NicEnsembleAdamState*": "c_void_p", "const int32_t*": "c_void_p", "NicTable2": "NicTable2",
           "int64_t": "c_long", "int32_t": "c_int"}


@pytest.mark.parametrize("name", sorted(ENTRY_POINTS))
def test_entry_points_are_declared_and_bound_argument_for_argument(name):
    with open(os.path.join(ROOT, "include", "nic_rollout.h")) as f:
        header = f.read()
    m = re.search(r"int %s\(([^)]*)\);" % name, header)
    assert m, f"{name} is not declared in include/nic_rollout.h"
    declared = [" ".join(a.split()).rsplit(" ", 1)[0] for a in m.group(1).split(",")]
    res, args = _lib.PROTOTYPES[name]
    assert res is _lib.C.c_int and len(args) == len(declared) == ENTRY_POINTS[name]
    assert [C_TYPES[d] for d in declared] == [a.__name__ for a in args], (declared, args)
    assert declared[-2:] == ["const int32_t*", "void*"]   # the mask is the one extra argument, ahead of the stream
    # ... and everything ahead of it is the unmasked entry point's list (the optimizer's pair is its own: one pair for both steps)
    if name.startswith("nic_small_rollout"):
        plain = re.search(r"int %s\(([^)]*)\);" % name[:-len("_active")], header)
        assert [" ".join(a.split()) for a in plain.group(1).split(",")] == \
            [" ".join(a.split()) for a in m.group(1).split(",")][:-2] + ["void* stream"]
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        assert name in f.read()
    assert hasattr(_lib.load_library(), name)
    assert "cannot be checked on the host" in header   # (the mask's contents: said where the entry points are declared)


def test_refused_without_a_device():
    """the mask's address is checked before anything touches the device"""
    lib = _lib.load_library()
    keep = torch.zeros(64)
    A = keep.data_ptr()
    assert lib.nic_ensemble_adam_prepare_active(3, 0, A, None, A, A, None, 0, None, A + 2, None) != 0
    message = lib.nic_last_error().decode()
    assert message.startswith("nic_ensemble_adam_prepare_active:") and MASK_REASON in message, message
    assert lib.nic_ensemble_adam_prepare_active(3, 8, A, A, A, A, None, 8, A, None, None) != 0
    assert "go together" in lib.nic_last_error().decode()
    assert lib.nic_ensemble_adam_update_active(3, 8, A, 8, A, 8, A, 8, A, 8, A, None, A + 1, None) != 0
    assert lib.nic_last_error().decode().startswith("nic_ensemble_adam_update_active:")
    ens = _lib.NicSmallEnsemble()
    ens.n_models, ens.rewards, ens.scratch = 3, 64, 4096
    assert lib.nic_small_rollout_ensemble_reduce_active(ens, None, 0, 0, 0, None, A, 64, 0, A, A, A + 3, None) != 0
    message = lib.nic_last_error().decode()
    assert message.startswith("nic_small_rollout_ensemble_reduce_active:") and MASK_REASON in message, message


# ---- the protocol: early_stopping_update against Trainer.train's own bookkeeping --------------------------------------------------------
class _TrainerBooks:
    """trainer.py:177-197 and :547-556 for ONE model, transcribed statement for statement without the rollouts: `train` gets the
    losses an epoch would have produced."""

    def __init__(self):
        self.best_performance_data = {"train_loss": math.inf, "dev_loss": math.inf}
        self.best_epoch = 0
        self.all_train_losses, self.all_dev_losses = [], []
        self.stopped_epoch = -1

    def update_best_params_and_save(self, epoch, train_loss, dev_loss, trainer_params):
        current = {"train_loss": train_loss, "dev_loss": dev_loss}
        key = trainer_params["choose_best_model_on"]
        if current[key] < self.best_performance_data[key]:
            self.best_performance_data["train_loss"] = train_loss
            self.best_performance_data["dev_loss"] = dev_loss
            self.best_epoch = epoch

    def train(self, epochs, train_losses, dev_losses, trainer_params):
        for epoch in range(epochs):
            train_report = train_losses[epoch]
            self.all_train_losses.append(train_report)
            if epoch % trainer_params["do_dev_every_n_epochs"] == 0:
                dev_report = dev_losses[epoch]
                self.all_dev_losses.append(dev_report)
                self.update_best_params_and_save(epoch, train_report, dev_report, trainer_params)
                patience = trainer_params.get("early_stopping_patience_epochs", None)
                if patience is not None and (epoch - self.best_epoch) >= patience:
                    self.stopped_epoch = epoch
                    break
            else:
                self.all_dev_losses.append(self.all_dev_losses[-1])


def _scripts(epochs, patience):
    """[K = 4][epochs] losses: never improves after the first epoch, improves every epoch, ties its best (strict <), and improves
    exactly `patience - 1` epochs after its best each time"""
    never = [5.0] + [6.0 + 0.25 * e for e in range(1, epochs)]
    always = [9.0 - 0.5 * e for e in range(epochs)]
    ties = [4.0] * epochs
    gap = max((patience or 4) - 1, 1)
    late, level = [], 8.0
    for e in range(epochs):
        if e % gap == 0:
            level -= 1.0
        late.append(level if e % gap == 0 else level + 3.0)
    return [never, always, ties, late]


def _drive(epochs, train, dev, trainer_params):
    """the engines' loop around `early_stopping_update` on CPU tensors: what `_fit_protocol` does with the losses"""
    K = len(train)
    every, _, patience = es.read_trainer_params(trainer_params)
    train_t, dev_t = torch.tensor(train, dtype=torch.float32), torch.tensor(dev, dtype=torch.float32)
    best_train, best_dev = torch.full((K,), math.inf), torch.full((K,), math.inf)
    best_epoch, stopped = torch.zeros(K, dtype=torch.int64), torch.full((K,), -1, dtype=torch.int64)
    active = torch.ones(K, dtype=torch.bool)
    lengths = torch.zeros(K, dtype=torch.int64)
    for epoch in range(epochs):
        lengths += active
        if epoch % every == 0:
            _, best_train, best_dev, best_epoch, still = es.early_stopping_update(train_t[:, epoch], dev_t[:, epoch], best_train, best_dev,
                                                                                  best_epoch, active, epoch, trainer_params)
            stopped = torch.where(active & ~still, torch.full_like(stopped, epoch), stopped)
            active = still
            if patience is not None and not bool(active.any()):
                break
    return best_train, best_dev, best_epoch, stopped, lengths


@pytest.mark.parametrize("every,choose,patience", list(itertools.product((1, 3), ("dev_loss", "train_loss"), (None, 1, 4))))
def test_protocol_function_is_trainer_train_per_model(every, choose, patience):
    epochs = 13
    trainer_params = {"do_dev_every_n_epochs": every, "choose_best_model_on": choose}
    if patience is not None:
        trainer_params["early_stopping_patience_epochs"] = patience
    chosen = _scripts(epochs, patience)
    other = [[v + 0.125 * ((e * 7 + m) % 5) for e, v in enumerate(row)] for m, row in enumerate(chosen)]   # (the loss that is not chosen on)
    train, dev = (other, chosen) if choose == "dev_loss" else (chosen, other)
    best_train, best_dev, best_epoch, stopped, lengths = _drive(epochs, train, dev, trainer_params)
    for m in range(4):
        ref = _TrainerBooks()
        ref.train(epochs, [float(torch.tensor(v, dtype=torch.float32)) for v in train[m]],
                  [float(torch.tensor(v, dtype=torch.float32)) for v in dev[m]], trainer_params)
        assert float(best_train[m]) == ref.best_performance_data["train_loss"], (m, "best train loss")
        assert float(best_dev[m]) == ref.best_performance_data["dev_loss"], (m, "best dev loss")
        assert int(best_epoch[m]) == ref.best_epoch, (m, "best epoch")
        assert int(stopped[m]) == ref.stopped_epoch, (m, "stop epoch")
        assert int(lengths[m]) == len(ref.all_train_losses) == len(ref.all_dev_losses), (m, "history length")
    if patience is not None:   # the scripts do what they are named for
        assert int(stopped[0]) >= 0 and int(best_epoch[0]) == 0      # never improves: stops, best at epoch 0
        assert int(best_epoch[2]) == 0                                # a tie is not an improvement
    if every == 1:
        assert int(stopped[1]) == -1 or patience == 0                 # improves every epoch: never stops


def test_protocol_function_leaves_inactive_models_alone_and_modifies_nothing_in_place():
    tp = {"do_dev_every_n_epochs": 1, "choose_best_model_on": "dev_loss", "early_stopping_patience_epochs": 2}
    train, dev = torch.tensor([1.0, 1.0, 1.0]), torch.tensor([0.5, 0.5, float("nan")])
    best_train, best_dev = torch.tensor([2.0, 2.0, 2.0]), torch.tensor([1.0, 1.0, 1.0])
    best_epoch, active = torch.tensor([3, 3, 3]), torch.tensor([True, False, True])
    keep = [t.clone() for t in (best_train, best_dev, best_epoch, active)]
    better, bt, bd, be, act = es.early_stopping_update(train, dev, best_train, best_dev, best_epoch, active, 5, tp)
    assert better.tolist() == [True, False, False]            # (inactive: not better; a NaN loss never is)
    assert bt.tolist() == [1.0, 2.0, 2.0] and bd.tolist() == [0.5, 1.0, 1.0] and be.tolist() == [5, 3, 3]
    assert act.tolist() == [True, False, False]               # model 2: 5 - 3 >= 2 stops it
    for t, k in zip((best_train, best_dev, best_epoch, active), keep):
        assert torch.equal(t, k)


def test_trainer_params_are_read_as_the_trainer_reads_them():
    assert es.read_trainer_params({"do_dev_every_n_epochs": 2, "choose_best_model_on": "train_loss"}) == (2, "train_loss", None)
    assert es.read_trainer_params({"do_dev_every_n_epochs": 1, "choose_best_model_on": "dev_loss",
                                   "early_stopping_patience_epochs": None, "save_model": True}) == (1, "dev_loss", None)
    with pytest.raises(KeyError):
        es.read_trainer_params({"choose_best_model_on": "dev_loss"})
    with pytest.raises(ValueError, match="choose_best_model_on"):
        es.read_trainer_params({"do_dev_every_n_epochs": 1, "choose_best_model_on": "test_loss"})
    with pytest.raises(ValueError, match="do_dev_every_n_epochs"):
        es.read_trainer_params({"do_dev_every_n_epochs": 0, "choose_best_model_on": "dev_loss"})


def test_fit_takes_trainer_params():
    import inspect
    assert inspect.signature(es.EnsembleStep.fit).parameters["trainer_params"].default is None
