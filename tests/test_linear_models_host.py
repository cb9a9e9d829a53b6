"""Host side of the model-batched GEMM entry points (nic_linear_fwd_models, nic_linear_wgrad_models, nic_wgrad_reduce_models): the
checks and plans of csrc/linear_models_plan.h through a stand-alone program built with the host compiler, the C declarations against
their ctypes prototypes, and the refusals of `HorizonPolicyEnsemble.train_step` that need no device."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest
import torch

from neural_inventory_control_amd import _lib, build, horizon_ensemble as he
from neural_inventory_control_amd.ensemble_adam import EnsembleAdam

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CUS = 256
(OK, MODELS, NULL, SIZES, ACT, LD, POINTER_ALIGN, SPLITS, NEGATIVE, Y_STRIDE, SLAB_STRIDE, DW_STRIDE, DB_STRIDE, W_STRIDE, BIAS_STRIDE,
 X_STRIDE, DY_STRIDE, ALIGN, PLAN) = range(19)


def _host_clang():
    hipcc = os.path.realpath(shutil.which(build._hipcc()) or build._hipcc())
    for c in (os.path.join(os.path.dirname(hipcc), "..", "llvm", "bin", "clang++"), "/opt/rocm/llvm/bin/clang++",
              shutil.which("clang++"), shutil.which("g++")):
        if c and os.path.isfile(c):
            return c
    raise RuntimeError("no host C++ compiler to build tests/linear_models_plan_harness.cpp")


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("linear_models_plan") / "harness")
    # (-Wall -Werror: the header has to stay clean C++ for a compiler that knows nothing of HIP)
    subprocess.run([_host_clang(), "-O1", "-std=c++17", "-Wall", "-Werror", "-o", exe,
                    os.path.join(ROOT, "tests", "linear_models_plan_harness.cpp")], check=True)

    def run(*args):
        return subprocess.run([exe] + [a if isinstance(a, str) else str(int(a)) for a in args], check=True, capture_output=True,
                              text=True).stdout.strip()
    return run


def _up4(n):
    return (n + 3) // 4 * 4


# ---- requests: a good one per entry point, fields overridden by name ---------------------------------------------------------------
def _fwd(harness, N=17, K=41, cols=140, cus=CUS, **kw):
    ldw, ldb = kw.get("ldw", _up4(K)), kw.get("ldb", cols)
    a = dict(W=256, bias=256, X=256, Y=256, ldw=ldw, W_stride=_up4(N * ldw) + 8, bias_stride=N + 3, X_stride=K * ldb + 8,
             Y_stride=N * ldb + 8, N=N, K=K, n_scenarios=cols, ldb=ldb, act=_lib.NIC_ACT_ELU, n_models=3)
    a.update(kw)
    return harness("fwd", *[a[k] for k in ("W", "bias", "X", "Y", "ldw", "W_stride", "bias_stride", "X_stride", "Y_stride", "N", "K",
                                           "n_scenarios", "ldb", "act", "n_models")], cus).split("|")


def _wgrad(harness, N=17, K=41, cols=140, **kw):
    ldb, lds, n_splits = kw.get("ldb", cols), kw.get("lds", _up4(K + 1)), kw.get("n_splits", 3)
    a = dict(dY=256, X=256, slab=256, dY_stride=N * ldb + 8, X_stride=K * ldb + 8, slab_stride=_up4(max(n_splits, 0) * N * lds) + 8, lds=lds,
             N=N, K=K, n_scenarios=cols, ldb=ldb, n_splits=n_splits, n_models=3)
    a.update(kw)
    return harness("wgrad", *[a[k] for k in ("dY", "X", "slab", "dY_stride", "X_stride", "slab_stride", "lds", "N", "K", "n_scenarios", "ldb",
                                             "n_splits", "n_models")]).split("|")


def _reduce(harness, N=17, K=41, **kw):
    lds, lddw, n_splits = kw.get("lds", _up4(K + 1)), kw.get("lddw", K), kw.get("n_splits", 3)
    a = dict(slab=256, dW=256, db=256, slab_stride=_up4(max(n_splits, 0) * N * lds) + 8, lds=lds, lddw=lddw, dW_stride=N * lddw + 5, db_stride=N + 3,
             N=N, K=K, n_splits=n_splits, n_models=3)
    a.update(kw)
    return harness("reduce", *[a[k] for k in ("slab", "dW", "db", "slab_stride", "lds", "lddw", "dW_stride", "db_stride", "N", "K", "n_splits",
                                              "n_models")]).split("|")


def _code(out):
    return int(out[0])


def test_accepted_requests_are_accepted(harness):
    assert _code(_fwd(harness)) == _code(_wgrad(harness)) == _code(_reduce(harness)) == OK
    for n in (1, 65535):
        assert _code(_fwd(harness, n_models=n)) == _code(_wgrad(harness, n_models=n)) == _code(_reduce(harness, n_models=n)) == OK
    # the exact slices; one shared input and no bias in the forward; no db in the reduction; free strides of the scalar operands
    assert _code(_fwd(harness, W_stride=17 * 44, X_stride=41 * 140, Y_stride=17 * 140, bias_stride=17)) == OK
    assert _code(_fwd(harness, X_stride=0)) == OK and _code(_fwd(harness, bias=0, bias_stride=0)) == OK
    assert _code(_fwd(harness, bias_stride=1234567)) == OK
    assert _code(_wgrad(harness, dY_stride=17 * 140, X_stride=41 * 140, slab_stride=3 * 17 * 44)) == OK
    assert _code(_reduce(harness, db=0, db_stride=0)) == OK and _code(_reduce(harness, dW_stride=16 * 41 + 41, db_stride=17)) == OK
    assert _code(_reduce(harness, dW_stride=1234567, db_stride=7654321)) == OK


def test_every_refusal_is_reached_with_its_reason(harness):
    reasons = dict((int(line.split("|")[0]), line.split("|")[1]) for line in harness("reasons").splitlines())
    assert sorted(reasons) == list(range(19)) and reasons[OK] == "accepted" and len(set(reasons.values())) == 19
    N, K, cols = 17, 41, 140
    cases = {
        MODELS: [_fwd(harness, n_models=0), _fwd(harness, n_models=65536), _wgrad(harness, n_models=-1), _reduce(harness, n_models=0)],
        NULL: [_fwd(harness, W=0), _fwd(harness, X=0), _fwd(harness, Y=0), _wgrad(harness, dY=0), _wgrad(harness, X=0), _wgrad(harness, slab=0),
               _reduce(harness, slab=0), _reduce(harness, dW=0)],
        SIZES: [_fwd(harness, N=0), _fwd(harness, ldw=K - 1), _wgrad(harness, lds=K), _wgrad(harness, K=0), _reduce(harness, lddw=K - 1),
                _reduce(harness, lds=K)],
        ACT: [_fwd(harness, act=2), _fwd(harness, act=-1)],
        LD: [_fwd(harness, ldb=cols + 2), _fwd(harness, ldb=cols - 4), _fwd(harness, cols=0, ldb=cols), _wgrad(harness, ldb=cols + 1)],
        POINTER_ALIGN: [_fwd(harness, X=260), _fwd(harness, Y=264)],
        SPLITS: [_wgrad(harness, n_splits=0), _reduce(harness, n_splits=-2)],
        NEGATIVE: [_fwd(harness, W_stride=-4), _fwd(harness, bias_stride=-1), _fwd(harness, X_stride=-4), _fwd(harness, Y_stride=-4),
                   _wgrad(harness, dY_stride=-4), _wgrad(harness, X_stride=-4), _wgrad(harness, slab_stride=-4),
                   _reduce(harness, slab_stride=-4), _reduce(harness, dW_stride=-1), _reduce(harness, db_stride=-1)],
        Y_STRIDE: [_fwd(harness, Y_stride=N * cols - 4), _fwd(harness, Y_stride=0)],
        SLAB_STRIDE: [_wgrad(harness, slab_stride=3 * N * 44 - 4), _reduce(harness, slab_stride=3 * N * 44 - 4), _reduce(harness, slab_stride=0)],
        DW_STRIDE: [_reduce(harness, dW_stride=(N - 1) * K + K - 1), _reduce(harness, dW_stride=0)],
        DB_STRIDE: [_reduce(harness, db_stride=N - 1), _reduce(harness, db_stride=0)],
        W_STRIDE: [_fwd(harness, W_stride=(N - 1) * 44 + K - 1), _fwd(harness, W_stride=0)],
        BIAS_STRIDE: [_fwd(harness, bias_stride=N - 1), _fwd(harness, bias_stride=0)],
        X_STRIDE: [_fwd(harness, X_stride=K * cols - 4), _wgrad(harness, X_stride=K * cols - 4), _wgrad(harness, X_stride=0)],
        DY_STRIDE: [_wgrad(harness, dY_stride=N * cols - 4), _wgrad(harness, dY_stride=0)],
        ALIGN: [_fwd(harness, W_stride=N * 44 + 2), _fwd(harness, X_stride=K * cols + 1), _fwd(harness, Y_stride=N * cols + 2),
                _wgrad(harness, dY_stride=N * cols + 2), _wgrad(harness, X_stride=K * cols + 3), _wgrad(harness, slab_stride=3 * N * 44 + 2),
                _reduce(harness, slab_stride=3 * N * 44 + 2)],
        PLAN: [_fwd(harness, N=512, K=512, cols=1024), _fwd(harness, N=65, K=41, cols=140), _fwd(harness, N=512, K=512, cols=65536),
               _wgrad(harness, N=129, K=33, cols=448), _wgrad(harness, N=128, K=256, cols=448)],
    }
    assert sorted(cases) == list(range(1, 19))
    for code, outs in cases.items():
        for out in outs:
            assert _code(out) == code and out[1] == reasons[code], (code, out)
    # 128 x 256 over 448 columns is an LDS-DMA shape (wgrad_mid): refused for its kernel, not for its height
    assert _wgrad(harness, N=128, K=256, cols=448)[2].split()[2] == "6"
    assert _code(_wgrad(harness, N=128, K=128, cols=448)) == OK


# (N, K, columns): the GPU test's shapes, the engine's real-data layers (observation share 64 x 576 and 64 x 22 over T * ldb columns,
# weight gradients 64 x 597, 64 x 64, 66 x 64, 64 x 30, 1 x 64), odd sizes around the tile edges
FWD_GRID = [(64, 462, 640), (64, 130, 640), (64, 22, 640), (17, 41, 140), (64, 576, 95 * 128), (64, 22, 95 * 8192), (1, 1, 4), (33, 127, 36),
            (32, 128, 4096), (64, 256, 2048), (31, 300, 100), (64, 64, 65536)]
WGRAD_GRID = [(32, 20), (17, 33), (32, 96), (32, 128), (32, 135), (64, 64), (33, 597), (66, 33), (66, 64), (64, 597), (66, 64), (64, 30),
              (1, 64), (128, 128), (65, 65), (128, 64), (1, 1)]


def test_the_model_plan_is_the_single_model_plan_for_model_0s_operands(harness):
    kernels = set()
    for N, K, cols in FWD_GRID:
        for cus in (256, 304, 64):
            for kw in (dict(), dict(ldw=K + 1 if (K + 1) % 4 else K + 2), dict(W=260), dict(ldb=cols + 8)):   # aligned; ldw % 4 != 0; W off 16 bytes
                out = _fwd(harness, N=N, K=K, cols=cols, cus=cus, **kw)
                assert _code(out) == OK, (N, K, cols, kw, out)
                assert out[2] == out[3]
                kernels.add(int(out[2].split()[1]))
    assert kernels == {0, 1, 3, 4, 6, 7}   # WX_STREAM_1x2, 1x4, WX_DMA_64x128, 32x128, WX_STAGED_64x128, 32x256
    tiles = set()
    for N, K in WGRAD_GRID:
        for cols in (140, 448, 95 * 128):
            for n_splits in (1, 3, 40):
                for kw in (dict(), dict(X=260), dict(lds=K + 2 if (K + 2) % 4 else K + 3)):
                    out = _wgrad(harness, N=N, K=K, cols=cols, n_splits=n_splits, **kw)
                    assert _code(out) == OK, (N, K, cols, kw, out)
                    assert out[2] == out[3] and int(out[2].split()[3]) == n_splits
                    tiles.add((int(out[2].split()[2]), int(out[2].split()[0])))
    # wgrad_small_kernel<1..4> (buffer operands only) and the four staged tiles, FAST and guarded
    assert tiles == {(t, 1) for t in (0, 1, 2, 3)} | {(t, b) for t in (11, 12, 13, 14) for b in (0, 1)}
    assert _reduce(harness, n_splits=130)[2] == "1" and _reduce(harness, n_splits=3)[2] == "0"
    assert _reduce(harness, N=512, K=512, n_splits=130)[2] == "0"
    # the model offset is 64-bit: the last model of the largest ensemble on a 2^31-float slice
    assert int(harness("offset", 65534, 2 ** 31)) == 65534 * 2 ** 31


def test_build_hashes_the_plan_header():
    assert "linear_models_plan.h" in build.HEADERS
    with open(os.path.join(build.CSRC, "linear_models_plan.h"), "rb") as f:
        text = f.read()
    with tempfile.TemporaryDirectory() as tmp:
        csrc = os.path.join(tmp, "pkg", "csrc")
        shutil.copytree(build.CSRC, csrc, ignore=shutil.ignore_patterns("*.o", "*.so", "*.key"))
        shutil.copytree(os.path.join(ROOT, "include"), os.path.join(tmp, "include"))
        assert build.source_id(csrc) == build.source_id()
        with open(os.path.join(csrc, "linear_models_plan.h"), "wb") as f:
            f.write(text + b"\n")
        assert build.source_id(csrc) != build.source_id()


ENTRY_POINTS = {"nic_linear_fwd_models": 16, "nic_linear_wgrad_models": 14, "nic_wgrad_reduce_models": 14, "nic_linear_models_ok": 6}
C_TYPES = {"float*": "c_void_p", "const float*": "c_void_p", "void*": "c_void_p", "int64_t": "c_long", "int32_t": "c_int", "float": "c_float"}


def _declared(header, name):
    m = re.search(r"int %s\(([^)]*)\);" % name, header)
    assert m, f"{name} is not declared in include/nic_rollout.h"
    return [" ".join(a.split()) for a in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")]


@pytest.mark.parametrize("name", sorted(ENTRY_POINTS))
def test_entry_points_are_declared_and_bound_argument_for_argument(name):
    with open(os.path.join(ROOT, "include", "nic_rollout.h")) as f:
        header = f.read()
    declared = [a.rsplit(" ", 1)[0] for a in _declared(header, name)]
    res, args = _lib.PROTOTYPES[name]
    assert res is _lib.C.c_int and len(args) == len(declared) == ENTRY_POINTS[name]
    assert [C_TYPES[d] for d in declared] == [a.__name__ for a in args], (declared, args)
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        assert name in f.read()
    assert hasattr(_lib.load_library(), name)


def test_model_calls_take_the_single_model_arguments_plus_strides():
    """every argument of the single-model call, in its order, each per-model buffer followed by its stride, n_models in front of the stream"""
    with open(os.path.join(ROOT, "include", "nic_rollout.h")) as f:
        header = f.read()
    for name, strides in (("nic_linear_fwd", ("W_stride", "bias_stride", "X_stride", "Y_stride")),
                          ("nic_linear_wgrad", ("dY_stride", "X_stride", "slab_stride")),
                          ("nic_wgrad_reduce", ("slab_stride", "dW_stride", "db_stride"))):
        one, many = _declared(header, name), _declared(header, name + "_models")
        extra = ["int64_t " + s for s in strides] + ["int32_t n_models"]
        assert [a for a in many if a not in extra] == one and sorted(a for a in many if a in extra) == sorted(extra)
        assert many[-2:] == ["int32_t n_models", "void* stream"]
        comment = header[:header.index("int %s_models(" % name)].rsplit("/*", 1)[1]
        assert "neural_networks.py:80-106" in comment and "once per model" in comment, name
    assert _lib.load_library().nic_abi_version() == 1


# ---- engine-side refusals that need no device ----------------------------------------------------------------------------------------
def _engine(k=2):
    from test_horizon_ensemble_host import _models
    models, _ = _models(k)
    ens = he.HorizonPolicyEnsemble.__new__(he.HorizonPolicyEnsemble)   # (the constructor asks for a device; nothing below launches)
    ens.models = he.check_models(models)
    ens._bind_requested = ens._bound = False
    return ens


def test_train_step_is_refused_without_bound_parameters_or_an_ensemble_adam():
    ens = _engine()
    with pytest.raises(ValueError, match=r"HorizonPolicyEnsemble.train_step needs bound parameters: call bind_parameters\(\) first"):
        ens.train_step({}, 5, optimizer=None)
    ens._bind_requested = True
    params = [p for m in ens.models for p in m.parameters()]
    for bad in (None, torch.optim.Adam(params, lr=1e-3), "adam"):
        with pytest.raises(ValueError, match="HorizonPolicyEnsemble.train_step needs an EnsembleAdam as `optimizer`"):
            ens.train_step({}, 5, optimizer=bad)
    # the optimizer's (K, P) against the engine's: checked on the host, in front of any launch
    ens.weights = torch.zeros(2, 10)
    opt = EnsembleAdam.__new__(EnsembleAdam)
    opt.n_models, opt.P = 3, 10
    with pytest.raises(ValueError, match="the optimizer is for 3 models of 10 parameters, the engine has 2 of 10"):
        ens._require_optimizer_shape(opt)
    opt.n_models = 2
    ens._require_optimizer_shape(opt)
    with pytest.raises(ValueError, match="load_best: no fit"):
        ens.best_weights = None
        ens.load_best()

