"""Opt-in bf16 GEMMs of the wide hidden layers (csrc/linear_bf16.hip, FusedRollout.gemm_precision = "bf16") on the GPU.

The kernels are checked against an EXACT emulation: operands rounded to bf16 by torch, contracted in fp64.  The only difference
the kernels may show is FP32 accumulation: |C - C_ref| <= n * 2^-24 * sum |a b| per element (n = terms of the contraction), plus
the rounding of the FP32 bias add and the ELU / ELU' epilogue.  A wrong lane map or a truncating conversion misses that by orders
of magnitude.  The engine in bf16 mode is compared with the FP32 engine (the parity-checked default) on the workloads' shapes."""
import copy
from collections import defaultdict

import pytest
import torch

from neural_inventory_control_amd import _lib, main_run, ops, workloads
from neural_inventory_control_amd.data_handling import Scenario
from neural_inventory_control_amd.loss_functions import PolicyLoss
from neural_inventory_control_amd.neural_networks import NeuralNetworkCreator
from neural_inventory_control_amd.rollout import FusedRollout

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24


def _bf(t):
    return t.to(torch.bfloat16).double()


def _elu(z):
    return torch.where(z > 0, z, torch.expm1(torch.clamp(z, max=0)))


def _rand(*shape, scale=1.0, gen=None):
    return (torch.randn(*shape, generator=gen, device=DEV) * scale).float()


def _within(got, ref, tol, what):
    err = (got.double() - ref).abs()
    worst = float((err / tol).max())
    assert worst <= 1.0, f"{what}: worst error / bound = {worst:.3g}"
    return worst


def _operands(N, K, nS, ldb, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    W = _rand(N, K, scale=K ** -0.5, gen=g)
    Wb = torch.zeros(N, (K + 31) // 32 * 32, dtype=torch.bfloat16, device=DEV)
    Wb[:, :K].copy_(W)
    X = torch.zeros(K, ldb, device=DEV)
    X[:, :nS] = _elu(_rand(K, nS, gen=g).double()).float()   # (an ELU activation, as the hidden layers see; padding columns 0)
    return W, Wb, X, g


SHAPES = [(512, 512, 1024, 1024), (512, 512, 8192, 8192), (512, 512, 65536, 65536), (512, 512, 1000, 1152), (256, 384, 4096, 4096)]


@pytest.mark.parametrize("N,K,nS,ldb", SHAPES)
def test_forward_against_exact_emulation(N, K, nS, ldb):
    W, Wb, X, g = _operands(N, K, nS, ldb, 1)
    bias = _rand(N, scale=0.1, gen=g)
    Y = torch.full((N, ldb), 12345.0, device=DEV)
    ops.linear_bf16_fwd(Wb[:, :K], bias, X, Y, nS, _lib.NIC_ACT_ELU)
    nc = (nS + 3) // 4 * 4
    a, b = _bf(W), _bf(X[:, :nc])
    z = a @ b
    S = a.abs() @ b.abs()
    zb = z + bias.double()[:, None]
    tol = K * U * S + 2 * U * zb.abs() + 3e-7 * (1 + zb.abs())   # accumulation + bias add + the ELU's approximation
    _within(Y[:, :nc], _elu(zb), tol, "forward")
    # padding columns: as the FP32 kernel leaves them
    Yf = torch.full((N, ldb), 12345.0, device=DEV)
    ops.linear_fwd(W, bias, X, Yf, nS, _lib.NIC_ACT_ELU)
    assert torch.equal(Y[:, nc:], Yf[:, nc:])
    # identity activation, no bias
    Y2 = torch.empty(N, ldb, device=DEV)
    ops.linear_bf16_fwd(Wb[:, :K], None, X, Y2, nS, _lib.NIC_ACT_NONE)
    _within(Y2[:, :nc], z, K * U * S + 1e-30, "forward (no bias, identity)")


@pytest.mark.parametrize("N,K,nS,ldb", SHAPES)
@pytest.mark.parametrize("accumulate", [0, 1])
def test_dgrad_against_exact_emulation(N, K, nS, ldb, accumulate):
    # dX[K][b] = (Wt[K][N] dY[N][b]) * ELU'(H[K][b]) (+ dX)
    W, _, _, g = _operands(N, K, 8, 8, 2)
    Wtb = torch.zeros(K, (N + 31) // 32 * 32, dtype=torch.bfloat16, device=DEV)
    Wtb[:, :N].copy_(W.t())
    dY = torch.zeros(N, ldb, device=DEV)
    dY[:, :nS] = _rand(N, nS, scale=1e-3, gen=g)
    H = _elu(_rand(K, ldb, gen=g).double()).float()
    prev = _rand(K, ldb, scale=1e-3, gen=g)
    dX = prev.clone()
    ops.linear_bf16_dgrad(Wtb[:, :N], dY, H, dX, nS, _lib.NIC_ACT_ELU, accumulate)
    nc = (nS + 3) // 4 * 4
    a, b = _bf(W.t()), _bf(dY[:, :nc])
    z = a @ b
    S = a.abs() @ b.abs()
    h = H[:, :nc].double()
    d = torch.where(h > 0, torch.ones_like(h), h + 1)
    ref = z * d + (prev[:, :nc].double() if accumulate else 0)
    tol = (N * U * S + 2 * U * z.abs()) * d + 2 * U * ref.abs() + 1e-30
    _within(dX[:, :nc], ref, tol, "dgrad")
    assert torch.equal(dX[:, nc:], prev[:, nc:])   # (the FP32 kernel writes columns < round_up(n, 4) only, too)


@pytest.mark.parametrize("N,K,nS,ldb", [(512, 512, 1024, 1024), (512, 512, 8192, 8192), (512, 512, 1000, 1152), (256, 384, 4096, 4096)])
def test_wgrad_against_exact_emulation(N, K, nS, ldb):
    g = torch.Generator(device=DEV).manual_seed(3)
    dY = _rand(N, ldb, scale=1e-3, gen=g)   # (padding columns hold garbage: they must not count)
    X = _rand(K, ldb, gen=g)
    splits = ops.wgrad_num_splits(N, K, nS)
    slab = torch.zeros(splits, N, (K + 1 + 3) // 4 * 4, device=DEV)
    ops.linear_bf16_wgrad(dY, X, slab, nS)
    ops.linear_bf16_wgrad(dY, X, slab, nS)   # (a second period adds to the slab)
    gw, gb = torch.empty(N, K, device=DEV), torch.empty(N, device=DEV)
    ops.wgrad_reduce(slab, gw, gb, K, 1.0)
    a, b = _bf(dY[:, :nS]), _bf(X[:, :nS])
    ref, S = 2 * (a @ b.t()), 2 * (a.abs() @ b.abs().t())
    _within(gw, ref, 2 * nS * U * S + 1e-30, "wgrad")
    dyd = dY[:, :nS].double()
    _within(gb, 2 * dyd.sum(1), 2 * nS * U * 2 * dyd.abs().sum(1) + 1e-30, "bias gradient")


@pytest.mark.parametrize("nS,ldb", [(1024, 1024), (1000, 1152)])
def test_wgrad_periods_against_exact_emulation(nS, ldb):
    # T = 7 periods; histories whose period strides are not the matrices' sizes ([T][N + 5][ldb] and [T][K + 3][ldb])
    N, K, T = 512, 512, 7
    g = torch.Generator(device=DEV).manual_seed(4)
    dYh = _rand(T, N + 5, ldb, scale=1e-3, gen=g)
    Xh = _rand(T, K + 3, ldb, gen=g)
    splits = ops.wgrad_periods_num_splits(N, K, nS, T)
    slab = torch.zeros(splits, N, (K + 1 + 3) // 4 * 4, device=DEV)
    ops.linear_bf16_wgrad_periods(dYh[:, :N], Xh[:, :K], slab, nS)
    gw, gb = torch.empty(N, K, device=DEV), torch.empty(N, device=DEV)
    ops.wgrad_reduce(slab, gw, gb, K, 1.0)
    a = _bf(dYh[:, :N, :nS]).permute(1, 0, 2).reshape(N, T * nS)
    b = _bf(Xh[:, :K, :nS]).permute(1, 0, 2).reshape(K, T * nS)
    _within(gw, a @ b.t(), T * nS * U * (a.abs() @ b.abs().t()) + 1e-30, "wgrad over periods")
    dyd = dYh[:, :N, :nS].double()
    _within(gb, dyd.sum((0, 2)), T * nS * U * dyd.abs().sum((0, 2)) + 1e-30, "bias gradient over periods")
    # determinism: the same launch again gives the same bits
    slab2 = torch.zeros_like(slab)
    ops.linear_bf16_wgrad_periods(dYh[:, :N], Xh[:, :K], slab2, nS)
    assert torch.equal(slab, slab2)


def test_kernels_deterministic():
    N, K, nS, ldb = 512, 512, 8192, 8192
    W, Wb, X, g = _operands(N, K, nS, ldb, 5)
    bias = _rand(N, gen=g)
    outs = []
    for _ in range(2):
        Y = torch.zeros(N, ldb, device=DEV)
        ops.linear_bf16_fwd(Wb[:, :K], bias, X, Y, nS, _lib.NIC_ACT_ELU)
        dX = torch.zeros(K, ldb, device=DEV)
        ops.linear_bf16_dgrad(Wb[:, :K], Y, X, dX, nS, _lib.NIC_ACT_ELU, 0)
        slab = torch.zeros(ops.wgrad_num_splits(N, K, nS), N, K + 4, device=DEV)
        ops.linear_bf16_wgrad(Y, X, slab, nS)
        outs.append((Y, dX, slab))
    for a, b in zip(*outs):
        assert torch.equal(a, b)


# ---- the engine ------------------------------------------------------------------------------------------------------------------

def _case(workload, n, T, seed=7):
    setting, policy, _, _, _ = workloads.get(workload)
    obs = defaultdict(lambda: None, setting["observation_params"])
    sc = Scenario(T, setting["problem_params"], setting["store_params"], setting["warehouse_params"], setting["echelon_params"], n,
                  obs, setting["seeds"], sampler="hip", device=DEV)
    data = {k: v.to(DEV) for k, v in sc.get_data().items()}
    torch.manual_seed(seed)
    model = NeuralNetworkCreator().create_neural_network(sc, policy, device=DEV)
    eng = FusedRollout(model, setting["problem_params"], DEV)
    eng.materialize(eng.input_rows(data, obs))
    return setting, data, model, eng, obs


def _engine(model, setting, data, obs, precision=None, **opts):
    eng = FusedRollout(model, setting["problem_params"], DEV)
    eng.materialize(eng.input_rows(data, obs))
    if precision is not None:
        eng.gemm_precision = precision
    for k, v in opts.items():
        setattr(eng, k, v)
    return eng


def _train(eng, data, T, obs):
    total, _ = eng.run(data, T, 0, train=True, observation_params=obs, assign_grads=False)
    torch.cuda.synchronize()
    return total.clone(), [g.clone() for _, g in eng.param_grads()]


def _hidden_512(model):
    lins = model.master_linears()
    return [i for i in range(1, len(lins) - 1) if lins[i].in_features == 512 and lins[i].out_features == 512]


@pytest.mark.parametrize("workload,n,T,route", [("cfg3", 1024, 10, "tail"), ("cfg3", 32768, 4, "per-period"), ("cfg5", 1024, 4, "any")])
def test_rollout_bf16_against_fp32(workload, n, T, route):
    """bf16 mode against the FP32 engine, same weights and batch.  The bars (total 5e-3 relative, per-parameter gradient cosine
    >= 0.98 and |dg| / |g| <= 0.2) were set from bf16's 2^-8 relative step before anything was measured.  Measured on MI355X at
    the initial weights: batch total within 1.0e-5 (cfg3, 1,024 x T=10), 1.9e-6 (cfg3, 32,768 x T=4), 2.7e-4 (cfg5, 1,024 x T=4);
    every gradient tensor cosine >= 0.99997 and |dg| / |g| = 0.003-0.008."""
    setting, data, model, _, obs = _case(workload, n, T)
    fp = _engine(model, setting, data, obs)
    bf = _engine(model, setting, data, obs, "bf16")
    t_fp, g_fp = _train(fp, data, T, obs)
    t_bf, g_bf = _train(bf, data, T, obs)
    assert bf.bf16_layers == _hidden_512(model) and len(bf.bf16_layers) == 2
    assert fp.bf16_layers == []
    if route == "tail":
        assert bf._use_tail() and bf._use_tail_bwd()
    elif route == "per-period":
        assert not bf._use_tail()
    rel = abs(float(t_bf) - float(t_fp)) / abs(float(t_fp))
    stats = {"total_rel": rel}
    assert rel <= 5e-3, stats
    for k, (a, b) in enumerate(zip(g_fp, g_bf)):
        a, b = a.double().flatten(), b.double().flatten()
        cos = float(a @ b / (a.norm() * b.norm()).clamp_min(1e-300))
        dn = float((a - b).norm() / a.norm().clamp_min(1e-300))
        stats[f"g{k}"] = (round(cos, 5), round(dn, 4))
        assert cos >= 0.98 and dn <= 0.2, stats
    e_fp, _ = fp.run(data, T, 0, train=False, observation_params=obs)
    e_bf, _ = bf.run(data, T, 0, train=False, observation_params=obs)
    assert bf.bf16_layers == _hidden_512(model)
    assert abs(float(e_bf) - float(e_fp)) <= 5e-3 * abs(float(e_fp))
    print(f"{workload} {n}x{T}: {stats}")


def test_bf16_training_step_deterministic():
    setting, data, model, _, obs = _case("cfg3", 1024, 4)
    eng = _engine(model, setting, data, obs, "bf16")
    t1, g1 = _train(eng, data, 4, obs)
    t2, g2 = _train(eng, data, 4, obs)
    assert torch.equal(t1, t2) and all(torch.equal(a, b) for a, b in zip(g1, g2))


def test_graph_replay_matches_eager_in_bf16():
    """use_graph=True against eager, three training steps with Adam steps in between: the bf16 weight copies are refreshed in place
    before every replay, so the replayed steps see the moved weights (bit-identical totals and gradients)."""
    setting, data, model, _, obs = _case("cfg3", 1024, 4)
    model2 = copy.deepcopy(model)
    runs = []
    for m, graph in ((model, False), (model2, True)):
        # (fuse_tail=True: the same backward launches in both modes; "auto" picks the per-layer ones under replay at 1,024)
        eng = _engine(m, setting, data, obs, "bf16", use_graph=graph, fuse_tail=True)
        opt = torch.optim.Adam(m.parameters(), lr=1e-3)
        seq = []
        for _ in range(3):
            opt.zero_grad()
            total, _ = eng.run(data, 4, 0, train=True, observation_params=obs)
            torch.cuda.synchronize()
            seq.append((total.clone(), [p.grad.clone() for p in m.parameters()]))
            opt.step()
        if graph:
            assert set(eng._graphs) == {"fwd", "bwd"}
        runs.append(seq)
    for (ta, ga), (tb, gb) in zip(*runs):
        assert torch.equal(ta, tb)
        assert all(torch.equal(a, b) for a, b in zip(ga, gb))


def test_no_eligible_layers_and_explicit_fp32_unchanged():
    # cfg1: the small whole-horizon route (32-wide policy) - bf16 changes nothing
    setting, data, model, _, obs = _case("cfg1", 256, 8)
    a = _engine(model, setting, data, obs, "fp32")
    b = _engine(model, setting, data, obs, "bf16")
    ta, ga = _train(a, data, 8, obs)
    tb, gb = _train(b, data, 8, obs)
    assert b.small is not None and b.bf16_layers == []
    assert torch.equal(ta, tb) and all(torch.equal(x, y) for x, y in zip(ga, gb))
    # cfg3 at 1,024 x T=4: explicit "fp32" is the default, bit for bit
    setting, data, model, _, obs = _case("cfg3", 1024, 4)
    a = _engine(model, setting, data, obs)
    b = _engine(model, setting, data, obs, "fp32")
    ta, ga = _train(a, data, 4, obs)
    tb, gb = _train(b, data, 4, obs)
    assert b.bf16_layers == []
    assert torch.equal(ta, tb) and all(torch.equal(x, y) for x, y in zip(ga, gb))


def test_invalid_precision_and_wide_route_refused():
    setting, data, model, _, obs = _case("cfg3", 1024, 2)
    eng = _engine(model, setting, data, obs, "fp16")
    with pytest.raises(ValueError):
        eng.run(data, 2, 0, train=True, observation_params=obs)
    eng = _engine(model, setting, data, obs, "bf16", use_wide=True)
    with pytest.raises(ValueError):
        eng.run(data, 2, 0, train=True, observation_params=obs)


def test_bf16_training_still_learns():
    """cfg3_yaml (the reference's shipped one-warehouse batch: 5 stores, batches of 1,024 x T=50): 40 epochs at each precision from
    the same initial weights and shuffling seed, then both final policies evaluated IN FP32 on the dev set.

    40, not 20: measured on MI355X (dev loss every 5 epochs, two shuffling seeds per precision), the dev loss falls from ~19 to
    ~5.4 between epochs 15 and 25, and at epoch 20 two FP32 runs that differ only in the shuffling seed stood at 6.77 and 9.78
    (bf16: 11.8 and 11.5) - a 1.02 bar there measures where each run is in that drop.  At epoch 40 all four runs are on the
    plateau: FP32 5.343 / 5.346, bf16 5.364 / 5.373 (ratio 1.004 / 1.005)."""
    setting, hyper, _ = workloads.get_epoch("cfg3_yaml")
    torch.manual_seed(11)
    c = main_run.build(setting, hyper, DEV)
    model, loaders, sim, pbd = c["model"], c["data_loaders"], c["simulator"], c["params_by_dataset"]
    pp, obs = c["problem_params"], c["observation_params"]
    lr = hyper["optimizer_params"]["learning_rate"]

    def dev_loss(tr):
        tr.gemm_precision = "fp32"
        _, rep = tr.do_one_epoch(None, loaders["dev"], PolicyLoss(), sim, model, pbd["dev"]["periods"], pp, obs, train=False,
                                 ignore_periods=pbd["dev"]["ignore_periods"])
        return rep

    from neural_inventory_control_amd.trainer import Trainer
    untrained = dev_loss(Trainer(device=DEV))   # (also materialises the lazy first layer)
    init = copy.deepcopy(model.state_dict())
    final = {}
    for precision in ("fp32", "bf16"):
        model.load_state_dict(init)
        opt = torch.optim.Adam(model.parameters(), lr=lr)
        tr = Trainer(device=DEV)
        tr.gemm_precision = precision
        torch.manual_seed(5)
        for _ in range(40):
            tr.do_one_epoch(opt, loaders["train"], PolicyLoss(), sim, model, pbd["train"]["periods"], pp, obs, train=True,
                            ignore_periods=pbd["train"]["ignore_periods"])
        if precision == "bf16":
            eng = tr._engines[(id(model), True)]
            assert eng.bf16_layers == _hidden_512(model)
        final[precision] = dev_loss(tr)
    print(f"dev loss: untrained {untrained}, fp32 {final['fp32']}, bf16 {final['bf16']}")
    assert final["fp32"] < untrained and final["bf16"] < untrained
    assert final["bf16"] <= 1.02 * final["fp32"]
