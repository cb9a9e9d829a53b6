"""The model-batched GEMM entry points (nic_linear_fwd_models, nic_linear_wgrad_models, nic_wgrad_reduce_models) against K calls of
the unchanged single-model entry points on each model's slice.  The bar is bit equality over the WHOLE output buffers: strides are the
slice + a gap of 8 floats, every gap and padding column of an output holds NaN, so anything written outside the live elements shows.
Shapes come from csrc/wx_plan.h / wgrad_plan.h so that every kernel with a model form is reached at its smallest."""
import re

import pytest
import torch

from neural_inventory_control_amd import _lib, ops

pytestmark = pytest.mark.gpu
GAP = 8
NAN = float("nan")


def _lib_stream():
    return _lib.lib(), _lib.current_stream()


def _p(t, off=0):
    return None if t is None else t.data_ptr() + 4 * off


def _rand(n, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randn(n, device="cuda", generator=g)


def _bits_equal(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def _kernel():
    return _lib.lib().nic_last_kernel().decode()


def _single_name(name):
    """the single-model kernel's name behind a model launch's"""
    return re.sub(r",models=\d+", "", name)


def _up4(n):
    return (n + 3) // 4 * 4


# ---- forward ---------------------------------------------------------------------------------------------------------------------
# (N, K, columns, ldw, act, with bias, X shared): per shape one case with ELU + bias + shared input, one without any of them
FWD_SHAPES = [(64, 462, 640, 464), (64, 130, 640, 132),          # streamed: 4 and 2 wavefronts split the contraction
              (64, 22, 640, 24),                                  # 64 x 128 LDS-DMA tile
              (17, 41, 140, 44),                                  # 32 x 128 tile, ragged columns (ldb = 20, 7 periods)
              (64, 22, 640, 23), (17, 41, 140, 41)]               # ldw % 4 != 0: the guarded staged tiles 64 x 128 and 32 x 256
FWD_CASES = [s + v for s in FWD_SHAPES for v in ((_lib.NIC_ACT_ELU, True, True), (_lib.NIC_ACT_NONE, False, False))]
FWD_KERNELS = {"gemm_wx_stream_kernel<1,4,EPI_BIAS_ACT>", "gemm_wx_stream_kernel<1,2,EPI_BIAS_ACT>",
               "gemm_wx_dma_kernel<2,4,1,1,EPI_BIAS_ACT>", "gemm_wx_dma_kernel<1,4,1,1,EPI_BIAS_ACT>",
               "gemm_wx_kernel<1,4,2,1,EPI_BIAS_ACT>", "gemm_wx_kernel<1,4,1,2,EPI_BIAS_ACT>"}


def _fwd_case(case, M):
    N, K, cols, ldw, act, with_bias, shared = case
    lib, stream = _lib_stream()
    ldb = cols + 8   # (padding columns behind the live ones: the outputs' must stay NaN)
    sW, sB, sX, sY = _up4(N * ldw) + GAP, N + 3, K * ldb + GAP, N * ldb + GAP
    W, X = 0.1 * _rand(M * sW, 1), _rand(M * sX, 2)
    bias = _rand(M * sB, 3) if with_bias else None
    Y, want = torch.full((M * sY,), NAN, device="cuda"), torch.full((M * sY,), NAN, device="cuda")
    singles = set()
    for m in range(M):
        _lib.check(lib.nic_linear_fwd(_p(W, m * sW), ldw, _p(bias, m * sB), _p(X, 0 if shared else m * sX), _p(want, m * sY), N, K,
                                      cols, ldb, act, stream))
        singles.add(_kernel())
    _lib.check(lib.nic_linear_fwd_models(_p(W), ldw, sW, _p(bias), sB, _p(X), 0 if shared else sX, _p(Y), sY, N, K, cols, ldb, act, M,
                                         stream))
    name = _kernel()
    assert singles == {_single_name(name)} and name.endswith(",models=%d>" % M), (name, singles)
    assert _bits_equal(Y, want)
    live = want.view(M, sY)[:, :N * ldb].view(M, N, ldb)
    assert not torch.isnan(live[:, :, :cols]).any()
    assert torch.isnan(want.view(M, sY)[:, N * ldb:]).all() and torch.isnan(live[:, :, _up4(cols):]).all()
    return _single_name(name)


@pytest.mark.parametrize("M", [1, 3])
@pytest.mark.parametrize("case", FWD_CASES, ids=lambda c: "x".join(str(v) for v in c))
def test_forward_is_the_single_model_call_on_every_slice(case, M):
    _fwd_case(case, M)


# ---- weight gradient -------------------------------------------------------------------------------------------------------------
# (N, K, X misaligned by one float)
WGRAD_SHAPES = [(32, 20, 0), (17, 33, 0), (32, 96, 0), (32, 128, 0),      # wgrad_small_kernel<1..4>
                (32, 135, 0),                                               # 32 x 256
                (64, 64, 0), (33, 597, 0),                                  # 64 x 128
                (66, 33, 0),                                                # 128 x 64
                (66, 64, 0),                                                # 128 x 128
                (32, 135, 1), (64, 64, 1), (66, 33, 1), (66, 64, 1)]        # a misaligned X: the guarded form of the four staged tiles
WGRAD_KERNELS = ({"wgrad_small_kernel<%d>" % kc for kc in (1, 2, 3, 4)}
                 | {"gemm_wgrad_kernel<%s,%d>" % (t, fast) for t in ("2,2,2,2", "2,2,2,1", "1,4,2,1", "1,4,1,2") for fast in (0, 1)})


def _wgrad_case(shape, M, cols, n_splits):
    N, K, off = shape
    lib, stream = _lib_stream()
    ldb, lds = cols, _up4(K + 1)
    if n_splits == 0:
        n_splits = ops.wgrad_num_splits(N, K, cols)
    s_dy, s_x, s_slab = N * ldb + GAP, K * ldb + GAP, n_splits * N * lds + GAP
    dY, Xbuf = _rand(M * s_dy, 4), _rand(M * s_x + 4, 5)
    # the contraction ADDS to the slab: non-zero values in the live elements, NaN in the padding columns and the gaps
    start = torch.full((M, s_slab), NAN, device="cuda")
    start[:, :n_splits * N * lds].view(M, n_splits * N, lds)[:, :, :K + 1] = _rand(M * n_splits * N * (K + 1), 6).view(M, n_splits * N, K + 1)
    slab, want = start.clone(), start.clone()
    singles = set()
    for m in range(M):
        _lib.check(lib.nic_linear_wgrad(_p(dY, m * s_dy), _p(Xbuf, off + m * s_x), _p(want, m * s_slab), lds, N, K, cols, ldb, n_splits,
                                        stream))
        singles.add(_kernel())
    _lib.check(lib.nic_linear_wgrad_models(_p(dY), s_dy, _p(Xbuf, off), s_x, _p(slab), s_slab, lds, N, K, cols, ldb, n_splits, M, stream))
    name = _kernel()
    assert singles == {_single_name(name)} and name.endswith(",models=%d>" % M), (name, singles)
    assert _bits_equal(slab, want)
    live = want[:, :n_splits * N * lds].view(M, n_splits * N, lds)
    assert not torch.isnan(live[:, :, :K + 1]).any() and not torch.equal(live[:, :, :K + 1], start[:, :n_splits * N * lds].view(M, -1, lds)[:, :, :K + 1])
    assert torch.isnan(live[:, :, K + 1:]).all() and torch.isnan(want[:, n_splits * N * lds:]).all()
    return _single_name(name)


@pytest.mark.parametrize("M", [1, 3])
@pytest.mark.parametrize("shape", WGRAD_SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_weight_gradient_is_the_single_model_call_on_every_slice(shape, M):
    for cols in (140, 448):
        for n_splits in (1, 3, 0):   # 0: nic_wgrad_num_splits' recommendation
            _wgrad_case(shape, M, cols, n_splits)


# ---- reduce ------------------------------------------------------------------------------------------------------------------------
def _reduce_case(M, n_splits, scale, with_db):
    N, K = 17, 33
    lib, stream = _lib_stream()
    lds, lddw = _up4(K + 1), K + 3
    s_slab, s_dw, s_db = n_splits * N * lds + GAP, N * lddw + 5, N + 3   # (the dW and db strides are free: no multiple of 4)
    slab = _rand(M * s_slab, 7)
    dW, dW_want = torch.full((M * s_dw,), NAN, device="cuda"), torch.full((M * s_dw,), NAN, device="cuda")
    db, db_want = (torch.full((M * s_db,), NAN, device="cuda"), torch.full((M * s_db,), NAN, device="cuda")) if with_db else (None, None)
    singles = set()
    for m in range(M):
        _lib.check(lib.nic_wgrad_reduce(_p(slab, m * s_slab), lds, n_splits, _p(dW_want, m * s_dw), lddw, _p(db_want, m * s_db), N, K, scale,
                                        stream))
        singles.add(_kernel())
    _lib.check(lib.nic_wgrad_reduce_models(_p(slab), s_slab, lds, n_splits, _p(dW), lddw, s_dw, _p(db), s_db, N, K, scale, M, stream))
    name = _kernel()
    assert singles == {_single_name(name)} and name.endswith(",models=%d" % M), (name, singles)
    assert _bits_equal(dW, dW_want)
    rows = dW_want.view(M, s_dw)[:, :N * lddw].view(M, N, lddw)
    assert not torch.isnan(rows[:, :, :K]).any() and torch.isnan(rows[:, :, K:]).all() and torch.isnan(dW_want.view(M, s_dw)[:, N * lddw:]).all()
    if with_db:
        assert _bits_equal(db, db_want)
        assert not torch.isnan(db_want.view(M, s_db)[:, :N]).any() and torch.isnan(db_want.view(M, s_db)[:, N:]).all()
    return _single_name(name)


@pytest.mark.parametrize("M", [1, 3])
@pytest.mark.parametrize("n_splits", [3, 130])
def test_reduce_is_the_single_model_call_on_every_slice(n_splits, M):
    for scale, with_db in ((1.0, True), (0.5, True), (0.5, False)):
        _reduce_case(M, n_splits, scale, with_db)


def test_every_kernel_with_a_model_form_is_reached_and_no_other():
    assert {_fwd_case(case, 3) for case in FWD_CASES} == FWD_KERNELS
    assert {_wgrad_case(shape, 3, 140, 3) for shape in WGRAD_SHAPES} == WGRAD_KERNELS
    assert {_reduce_case(3, n, 1.0, True) for n in (3, 130)} == {"wgrad_reduce_kernel", "wgrad_reduce_wide_kernel"}


def test_the_ops_wrappers_take_the_strides_from_the_tensors():
    M, N, K, cols = 3, 17, 41, 140
    W, bias, X = 0.1 * _rand(M * N * 44, 8).view(M, N, 44), _rand(M * N, 9).view(M, N), _rand(M * K * cols, 10).view(M, K, cols)
    Y, want = torch.zeros(M, N, cols, device="cuda"), torch.zeros(M, N, cols, device="cuda")
    ops.linear_fwd_models(W[:, :, :K], bias, X[0], Y, cols, _lib.NIC_ACT_ELU)
    for m in range(M):
        ops.linear_fwd(W[m, :, :K], bias[m], X[0], want[m], cols, _lib.NIC_ACT_ELU)
    assert _bits_equal(Y, want)
    assert ops.linear_models_ok(N, K, cols, cols, M) and ops.linear_models_ok(N, K, cols, cols, M, wgrad=True)
    assert not ops.linear_models_ok(512, 512, 1024, 1024, M) and not ops.linear_models_ok(130, 33, 448, 448, M, wgrad=True)
    splits = ops.wgrad_num_splits(N, K, cols)
    dY = _rand(M * N * cols, 11).view(M, N, cols)
    slab, slab_want = torch.zeros(M, splits, N, 44, device="cuda"), torch.zeros(M, splits, N, 44, device="cuda")
    grad, grad_want = torch.zeros(M, N * K + N + 5, device="cuda"), torch.zeros(M, N * K + N + 5, device="cuda")
    ops.linear_wgrad_models(dY, X, slab, cols)
    ops.wgrad_reduce_models(slab, grad[0, :N * K].view(N, K), grad[0, N * K:N * K + N], K, 0.5, dW_stride=grad.stride(0),
                            db_stride=grad.stride(0))
    for m in range(M):
        ops.linear_wgrad(dY[m], X[m], slab_want[m], cols)
        ops.wgrad_reduce(slab_want[m], grad_want[m, :N * K].view(N, K), grad_want[m, N * K:N * K + N], K, 0.5)
    assert _bits_equal(slab, slab_want) and _bits_equal(grad, grad_want) and grad.abs().sum() > 0


# the reason of every refusal, as csrc/linear_models_plan.h words it (nic_last_error: "<entry point>: <reason>")
REASONS = {
    "models": "n_models must be 1..65535",
    "null": "null buffer",
    "sizes": "bad N / K / leading dimension of the weights, the slab or dW",
    "act": "unknown activation",
    "ld": "ldb must be a multiple of 4 and >= n_scenarios > 0",
    "pointer_align": "X / Y must be 16-byte aligned",
    "splits": "n_splits must be >= 1",
    "negative": "negative stride",
    "y_stride": "Y stride shorter than N * ldb",
    "slab_stride": "slab stride shorter than n_splits * N * lds",
    "dw_stride": "dW stride shorter than (N - 1) * lddw + K",
    "db_stride": "db stride shorter than N",
    "w_stride": "W stride shorter than (N - 1) * ldw + K",
    "bias_stride": "bias stride shorter than N",
    "x_stride": "X stride shorter than K * ldb (0, one shared input, is taken by the forward only)",
    "dy_stride": "dY stride shorter than N * ldb",
    "align": "the strides of W, X, Y, dY and the slab must be multiples of 4 floats",
    "plan": "the plan picks a kernel without a model form (forward: N <= 64; weight gradient: N <= 128, staged or small tiles)",
}


# ---- refusals: non-zero status, the reason in nic_last_error, nothing written; then a good request on the same buffers works -------
def test_refusals_launch_nothing_and_name_their_reason():
    lib, stream = _lib_stream()
    M, N, K, cols = 3, 17, 41, 140
    ldw, ldb, lds, lddw, n_splits = 44, cols, 44, K, 3
    sW, sB, sX, sY = N * ldw + GAP, N + 3, K * ldb + GAP, N * ldb + GAP
    s_slab, s_dw, s_db = n_splits * N * lds + GAP, N * lddw + 5, N + 3
    W, bias, X, dY = 0.1 * _rand(M * sW, 12), _rand(M * sB, 13), _rand(M * sX + 4, 14), _rand(M * sY, 15)
    nan = lambda n: torch.full((n,), NAN, device="cuda")   # noqa: E731
    Y, slab, dW, db = nan(M * sY), nan(M * s_slab), nan(M * s_dw), nan(M * s_db)
    outputs = (Y, slab, dW, db)

    def fwd(**kw):
        a = dict(W=_p(W), ldw=ldw, sW=sW, bias=_p(bias), sB=sB, X=_p(X), sX=sX, Y=_p(Y), sY=sY, N=N, K=K, cols=cols, ldb=ldb,
                 act=_lib.NIC_ACT_ELU, M=M)
        a.update(kw)
        return "nic_linear_fwd_models", lib.nic_linear_fwd_models(a["W"], a["ldw"], a["sW"], a["bias"], a["sB"], a["X"], a["sX"], a["Y"],
                                                                  a["sY"], a["N"], a["K"], a["cols"], a["ldb"], a["act"], a["M"], stream)

    def wgrad(**kw):
        a = dict(dY=_p(dY), s_dy=sY, X=_p(X), sX=sX, slab=_p(slab), s_slab=s_slab, lds=lds, N=N, K=K, cols=cols, ldb=ldb,
                 n_splits=n_splits, M=M)
        a.update(kw)
        return "nic_linear_wgrad_models", lib.nic_linear_wgrad_models(a["dY"], a["s_dy"], a["X"], a["sX"], a["slab"], a["s_slab"], a["lds"],
                                                                      a["N"], a["K"], a["cols"], a["ldb"], a["n_splits"], a["M"], stream)

    def reduce(**kw):
        a = dict(slab=_p(slab), s_slab=s_slab, lds=lds, n_splits=n_splits, dW=_p(dW), lddw=lddw, s_dw=s_dw, db=_p(db), s_db=s_db, N=N,
                 K=K, M=M)
        a.update(kw)
        return "nic_wgrad_reduce_models", lib.nic_wgrad_reduce_models(a["slab"], a["s_slab"], a["lds"], a["n_splits"], a["dW"], a["lddw"],
                                                                      a["s_dw"], a["db"], a["s_db"], a["N"], a["K"], 1.0, a["M"], stream)

    refused = [
        (fwd, dict(M=0), "models"), (wgrad, dict(M=65536), "models"), (reduce, dict(M=-1), "models"),
        (fwd, dict(W=None), "null"), (wgrad, dict(slab=None), "null"), (reduce, dict(dW=None), "null"),
        (fwd, dict(ldw=K - 1), "sizes"), (wgrad, dict(lds=K), "sizes"), (reduce, dict(lddw=K - 1), "sizes"),
        (fwd, dict(act=7), "act"),
        (fwd, dict(ldb=cols + 2), "ld"), (wgrad, dict(ldb=cols - 4), "ld"),
        (fwd, dict(X=_p(X, 1)), "pointer_align"),
        (wgrad, dict(n_splits=0), "splits"), (reduce, dict(n_splits=0), "splits"),
        (fwd, dict(sW=-4), "negative"), (wgrad, dict(s_dy=-4), "negative"), (reduce, dict(s_db=-1), "negative"),
        (fwd, dict(sY=N * ldb - 4), "y_stride"),
        (wgrad, dict(s_slab=n_splits * N * lds - 4), "slab_stride"), (reduce, dict(s_slab=n_splits * N * lds - 4), "slab_stride"),
        (reduce, dict(s_dw=(N - 1) * lddw + K - 1), "dw_stride"), (reduce, dict(s_db=N - 1), "db_stride"),
        (fwd, dict(sW=(N - 1) * ldw + K - 1), "w_stride"), (fwd, dict(sB=N - 1), "bias_stride"),
        (fwd, dict(sX=K * ldb - 4), "x_stride"), (wgrad, dict(sX=0), "x_stride"),
        (wgrad, dict(s_dy=N * ldb - 4), "dy_stride"),
        (fwd, dict(sY=sY + 2), "align"), (fwd, dict(sW=sW + 1), "align"), (wgrad, dict(sX=sX + 2), "align"),
        (reduce, dict(s_slab=s_slab + 2), "align"),
    ]
    assert {key for _, _, key in refused} == set(REASONS) - {"plan"}   # (the plan's refusal: the next test)
    for call, kw, key in refused:
        who, status = call(**kw)
        # (the message is the calling thread's last one: read right after the call, the entry point's name and the whole reason)
        assert status != 0 and lib.nic_last_error().decode() == "%s: %s" % (who, REASONS[key]), (kw, key, lib.nic_last_error())
    torch.cuda.synchronize()
    for t in outputs:
        assert torch.isnan(t).all()
    # the same buffers, good requests
    slab.zero_()
    assert fwd()[1] == 0 and wgrad()[1] == 0 and reduce()[1] == 0, lib.nic_last_error()
    torch.cuda.synchronize()
    assert not torch.isnan(Y.view(M, sY)[:, :N * ldb]).any() and torch.isnan(Y.view(M, sY)[:, N * ldb:]).all()
    assert not torch.isnan(dW.view(M, s_dw)[:, :N * lddw]).any() and not torch.isnan(db.view(M, s_db)[:, :N]).any()


def test_a_plan_without_a_model_form_is_refused():
    """512 x 512 over 1,024 columns: nic_linear_fwd streams it, but N > 64 is outside what the model forms cover; a weight gradient of
    130 rows likewise"""
    lib, stream = _lib_stream()
    M, N, K, cols = 2, 512, 512, 1024
    W, X, Y = 0.1 * _rand(M * N * K, 16), _rand(K * cols, 17), torch.full((M * N * cols,), NAN, device="cuda")
    assert lib.nic_linear_fwd_models(_p(W), K, N * K, None, 0, _p(X), 0, _p(Y), N * cols, N, K, cols, cols, _lib.NIC_ACT_ELU, M, stream) != 0
    assert lib.nic_last_error().decode() == "nic_linear_fwd_models: " + REASONS["plan"]
    N2, K2, cols2, lds = 130, 33, 448, 36
    dY, slab = _rand(M * N2 * cols2, 18), torch.full((M * N2 * lds,), NAN, device="cuda")
    assert lib.nic_linear_wgrad_models(_p(dY), N2 * cols2, _p(X), K2 * cols2, _p(slab), N2 * lds, lds, N2, K2, cols2, cols2, 1, M, stream) != 0
    assert lib.nic_last_error().decode() == "nic_linear_wgrad_models: " + REASONS["plan"]
    torch.cuda.synchronize()
    assert torch.isnan(Y).all() and torch.isnan(slab).all()
