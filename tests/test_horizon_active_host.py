"""Host side of skipping stopped models in the data_driven K-model launches: the mask checks of csrc/horizon_ensemble_plan.h and
csrc/linear_models_plan.h through a stand-alone program built with the host compiler alone, the seven `_active` entry points in
the header, the ctypes table and the built library, and the defaults of the Python layer (`skip_inactive`, `active=None`).  No
device."""
import ctypes
import inspect
import os
import re
import subprocess

import pytest

from neural_inventory_control_amd import _lib, build, ensemble_step, horizon_ensemble as he, horizon_rollout as hz, ops
from test_horizon_ensemble_host import _host_clang

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HORIZON_ACTIVE = ("nic_horizon_rollout_ensemble_fwd_active", "nic_horizon_rollout_ensemble_bwd_active",
                  "nic_horizon_rollout_instances_fwd_active", "nic_horizon_rollout_instances_bwd_active")
LINEAR_ACTIVE = ("nic_linear_fwd_models_active", "nic_linear_wgrad_models_active", "nic_wgrad_reduce_models_active")
MASK_REASON = "the active mask must be NULL or 4-byte aligned"
# every refusal that existed before the mask, with its value and its text
HE_REASONS = [
    "accepted", "n_models must be 1..65535", "only head_mode 0 (the MLP) has an ensemble form: a tape has no weights",
    "rounded orders have no gradient (evaluation only)", "negative stride", "W1 stride shorter than H1 * ldw1",
    "W2 stride shorter than H2 * ldw2", "W3 stride shorter than n_out * ldw3", "b2 stride shorter than H2", "b3 stride shorter than n_out",
    "z1_obs stride shorter than H1 * hist_stride", "rewards stride shorter than T * ldb",
    "final-state stride shorter than the state rows x ldb", "state-history stride shorter than its slice",
    "h1-history stride shorter than its slice", "h2-history stride shorter than its slice", "logits-history stride shorter than its slice",
    "orders-history stride shorter than its slice", "dz1 stride shorter than its slice", "dz2 stride shorter than its slice",
    "dz3 stride shorter than its slice",
    "the strides of z1_obs, the rewards, the final state, the histories and the dz buffers must be multiples of 4 floats"]
LM_REASONS = [
    "accepted", "n_models must be 1..65535", "null buffer", "bad N / K / leading dimension of the weights, the slab or dW",
    "unknown activation", "ldb must be a multiple of 4 and >= n_scenarios > 0", "X / Y must be 16-byte aligned", "n_splits must be >= 1",
    "negative stride", "Y stride shorter than N * ldb", "slab stride shorter than n_splits * N * lds",
    "dW stride shorter than (N - 1) * lddw + K", "db stride shorter than N", "W stride shorter than (N - 1) * ldw + K",
    "bias stride shorter than N", "X stride shorter than K * ldb (0, one shared input, is taken by the forward only)",
    "dY stride shorter than N * ldb", "the strides of W, X, Y, dY and the slab must be multiples of 4 floats",
    "the plan picks a kernel without a model form (forward: N <= 64; weight gradient: N <= 128, staged or small tiles)"]


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("horizon_active_plan") / "harness")
    # (-Wall -Werror: both headers have to stay clean C++ for a compiler that knows nothing of HIP)
    subprocess.run([_host_clang(), "-O1", "-std=c++17", "-Wall", "-Werror", "-o", exe,
                    os.path.join(ROOT, "tests", "horizon_active_plan_harness.cpp")], check=True)

    def run(*args):
        return subprocess.run([exe] + [a if isinstance(a, str) else str(int(a)) for a in args], check=True, capture_output=True,
                              text=True).stdout.strip()
    return run


def _answer(line):
    code, reason = line.split("|")
    return int(code), reason


# ---- the checks -----------------------------------------------------------------------------------------------------------------------
def test_horizon_mask_is_null_or_four_byte_aligned(harness):
    he_active = len(HE_REASONS)   # the new refusal follows the old ones
    for address in (0, 4, 4096, 4100, (1 << 40) + 8):   # NULL is taken, as small_ensemble_check_active takes it: every model runs
        assert _answer(harness("he_active", address)) == (0, "accepted"), address
    for address in (1, 2, 3, 4097, 4098, 4103, (1 << 40) + 6):
        assert _answer(harness("he_active", address)) == (he_active, MASK_REASON), address


def test_a_model_runs_unless_its_entry_is_zero(harness):
    # mask {1, 0, 7}: (horizon under the mask, horizon under NULL, linear under the mask, linear under NULL) per model
    assert harness("he_runs").splitlines() == ["1 1 1 1", "0 1 0 1", "1 1 1 1"]


def test_every_existing_refusal_keeps_its_value_and_text(harness):
    got = [_answer(line) for line in harness("he_reasons").splitlines()]
    assert got == list(enumerate(HE_REASONS + [MASK_REASON]))
    lines = harness("lm_reasons").splitlines()
    assert [_answer(line) for line in lines[:-1]] == list(enumerate(LM_REASONS + [MASK_REASON]))
    # LM_REFUSAL_END stays the end of what a request without a mask can be refused for; the mask's refusal follows it
    assert lines[-1] == "end|%d|%d" % (len(LM_REASONS), len(LM_REASONS) + 1)


@pytest.mark.parametrize("check", ["lm_fwd", "lm_wgrad", "lm_reduce"])
def test_linear_model_checks_take_an_aligned_or_null_mask_only(harness, check):
    lm_mask = len(LM_REASONS)
    for address in (0, 4, 16388):
        assert _answer(harness(check, address)) == (0, "accepted"), address
    for address in (1, 2, 16386, 16391):
        assert _answer(harness(check, address)) == (lm_mask, MASK_REASON), address
    # an argument error of the unmasked call is still what a request is refused for first, with its own code
    bad = {"lm_fwd": (17 * 140 - 4, 9), "lm_wgrad": (0, 15), "lm_reduce": (0, 7)}[check]
    for address in (0, 4, 2):
        assert _answer(harness(check, address, bad[0])) == (bad[1], LM_REASONS[bad[1]]), address


def test_the_plans_refuse_a_misaligned_mask_before_planning(harness):
    assert harness("lm_plans", 0) == "0|0" and harness("lm_plans", 64) == "0|0"
    assert harness("lm_plans", 66) == "%d|%d" % (len(LM_REASONS), len(LM_REASONS))


# ---- the ABI --------------------------------------------------------------------------------------------------------------------------
def _declaration(text, name):
    m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, text, re.S)
    assert m, name + " is not declared in include/nic_rollout.h"
    return [a.strip() for a in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")]


def test_the_seven_entry_points_are_declared_bound_and_exported():
    with open(os.path.join(ROOT, "include", "nic_rollout.h")) as f:
        header = f.read()
    lib_path = os.path.join(build.CSRC, "libnic_hip.so")
    assert os.path.isfile(lib_path), "build() has not run"
    symbols = subprocess.run(["nm", "-D", "--defined-only", lib_path], check=True, capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in symbols.splitlines() if line.strip()}
    for name in HORIZON_ACTIVE + LINEAR_ACTIVE:
        parent = name[:-len("_active")]
        args, parent_args = _declaration(header, name), _declaration(header, parent)
        # the entry point it is named after, with `const int32_t* active` ahead of the stream
        assert args[:-2] == parent_args[:-1] and args[-1] == parent_args[-1] == "void* stream", name
        assert re.fullmatch(r"const\s+int32_t\s*\*\s*active", args[-2]), (name, args[-2])
        (restype, argtypes), (_, p_argtypes) = _lib.PROTOTYPES[name], _lib.PROTOTYPES[parent]
        assert restype is ctypes.c_int and list(argtypes) == list(p_argtypes[:-1]) + [ctypes.c_void_p, ctypes.c_void_p], name
        assert len(argtypes) == len(args)
        assert name in exported and parent in exported, name


# ---- the Python layer's defaults ---------------------------------------------------------------------------------------------------------
def test_wrappers_take_no_mask_by_default():
    for fn in (hz.horizon_ensemble_fwd, hz.horizon_ensemble_bwd, hz.horizon_instances_fwd, hz.horizon_instances_bwd,
               ops.linear_fwd_models, ops.linear_wgrad_models, ops.wgrad_reduce_models):
        p = inspect.signature(fn).parameters
        assert "active" in p and p["active"].default is None, fn.__name__
        assert list(p)[-1] == "active", fn.__name__   # (behind everything the callers already pass)


def test_skipping_is_opt_in_on_the_horizon_engine():
    src = inspect.getsource(he.HorizonPolicyEnsemble.__init__)
    assert re.search(r"self\.skip_inactive\s*=\s*False\b", src)
    # a plain attribute: no property, nothing on the shared base (SmallPolicyEnsemble always skips)
    assert not hasattr(he.HorizonPolicyEnsemble, "skip_inactive") and not hasattr(ensemble_step.EnsembleStep, "skip_inactive")
    assert "the follow-up" not in (he.__doc__ + ensemble_step.__doc__)


def test_fit_protocol_switches_skipping_on_and_puts_the_previous_value_back():
    """`_fit_protocol` on a stand-in engine (no device, no library): `skip_inactive` is True while the epochs run and the previous
    value afterwards, also when an epoch raises; an engine without the attribute gets none."""
    seen = []

    class Engine(ensemble_step.EnsembleStep):
        def __init__(self, with_attribute, value=False, fail=False):   # (no base __init__: it asks for a device)
            if with_attribute:
                self.skip_inactive = value
            self.fail = fail

        def _protocol_epochs(self, *args):
            seen.append(getattr(self, "skip_inactive", None))
            if self.fail:
                raise RuntimeError("an epoch failed")
            return "train", "dev"

    params = {"do_dev_every_n_epochs": 1, "choose_best_model_on": "dev_loss", "early_stopping_patience_epochs": 2}
    for previous in (False, True):
        e = Engine(True, previous)
        assert e._fit_protocol([], [], 1, 1, 1, 0, None, None, params) == ("train", "dev")
        assert seen[-1] is True and e.skip_inactive is previous
    e = Engine(True, False, fail=True)
    with pytest.raises(RuntimeError, match="an epoch failed"):
        e._fit_protocol([], [], 1, 1, 1, 0, None, None, params)
    assert seen[-1] is True and e.skip_inactive is False
    e = Engine(False)
    e._fit_protocol([], [], 1, 1, 1, 0, None, None, params)
    assert seen[-1] is None and not hasattr(e, "skip_inactive")
