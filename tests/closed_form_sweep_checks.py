"""Shared by the CPU and GPU tests of the closed-form sweep (`closed_form_sweep_chain` / `nic_closed_form_sweep`): the inputs of a
case, candidate level vectors around its own levels, and both launches behind one signature, so that a candidate's numbers are
compared with a single-candidate run of the SAME backend (host build against host build, kernel against kernel)."""
import ctypes as C

import torch

import closed_form_checks as cfc
from golden_io import Golden
from neural_inventory_control_amd import _lib, closed_form as cf
from neural_inventory_control_amd.layout import EnvProblem

SCALES_5 = (0.5, 0.8, 1.0, 1.3, 2.0)     # row 2 = the case's own levels
SCALES_9 = (0.5, 0.65, 1.0, 0.8, 1.15, 1.3, 1.6, 2.0, 0.9)


class Case:
    """Device-side inputs of one rollout: problem, policy name, T, ignore_periods, levels [L], demand [T][S][ld], state0."""

    def __init__(self, prob, policy, T, ignore, levels, demand, state0, B, golden=None):
        self.prob, self.policy, self.T, self.ignore, self.levels = prob, policy, T, ignore, levels
        self.demand, self.state0, self.B, self.golden = demand, state0, B, golden

    def desc(self, levels, round_orders=False):
        return cf.make_desc(self.prob, self.policy, self.T, 0, self.ignore, levels, self.demand, self.state0, round_orders)

    def candidates(self, scales):
        return (self.levels[None, :] * torch.tensor(scales, device=self.levels.device)[:, None]).contiguous()


def make_case(problem_params, data, policy, T, ignore, levels, dev, golden=None):
    data = {k: v.to(dev) for k, v in data.items()}
    prob = EnvProblem(problem_params, data, dev)
    assert cf.supports_shapes(policy, prob)
    B = data["demands"].shape[0]
    demand = torch.zeros(data["demands"].shape[2], prob.S, prob.ldb, device=dev)
    demand[:, :, :B] = data["demands"].permute(2, 1, 0)
    return Case(prob, policy, T, ignore, levels.detach().float().contiguous().to(dev), demand, cf.pack_state0(data, prob), B, golden)


def golden_case(name, dev):
    g = Golden(name)
    c = g.fresh_config()
    levels, _ = cfc.levels_from_params(c["nn_params"], g.params)
    return make_case(c["problem_params"], g.data, c["policy"], c["periods"], c["ignore"], levels, dev, g)


def serial_case(seed, dev):
    s, nn, pol, data, obs, n, T = cfc.random_serial_case(seed)
    params = {"net.master.0.weight": pol.layers[0][0].detach(), "net.master.0.bias": pol.layers[0][1].detach()}
    levels, _ = cfc.levels_from_params(nn, params)
    return make_case(s["problem_params"], data, "echelon_stock", T, 0, levels, dev)


# ---- host build: (per-chain totals [2][S][ld], level gradient [L] float64 or None) ----------------------------------------------

def host_single(h, case, levels, want_grad):
    S, ld, L = case.prob.S, case.prob.ldb, levels.numel()
    totals = torch.zeros(2, S, ld)
    g = (C.c_double * L)() if want_grad else None
    h.hostsim_closed_form_rollout(case.desc(levels), None, totals.data_ptr(), None, g)
    return totals, (torch.tensor(list(g), dtype=torch.float64) if want_grad else None)


def host_sweep(hs, case, levels, kc, want_grad):
    K, L = levels.shape
    totals = torch.zeros(K, 2, case.prob.S, case.prob.ldb)
    g = (C.c_double * (K * L))() if want_grad else None
    assert hs.hostsim_closed_form_sweep(case.desc(levels[0]), levels.data_ptr(), K, kc, totals.data_ptr(), g) == 0
    return totals, (torch.tensor(list(g), dtype=torch.float64).reshape(K, L) if want_grad else None)


# ---- HIP kernels through the C ABI: (per-chain totals, per-wavefront partial rows) ---------------------------------------------

def hip_single(case, levels, want_grad, round_orders=False):
    S, ld, L = case.prob.S, case.prob.ldb, levels.numel()
    ng = L if want_grad else 0
    totals = torch.zeros(2, S, ld, device=levels.device)
    part = torch.zeros(_lib.lib().nic_closed_form_num_partials(case.B, S), ng + 2, device=levels.device)
    _lib.check(_lib.lib().nic_closed_form_rollout_sums(case.desc(levels, round_orders), None, totals.data_ptr(), None, part.data_ptr(),
                                                       ng + 2, int(want_grad), 1, _lib.current_stream()))
    torch.cuda.synchronize()
    return totals, part


def hip_sweep(case, levels, want_grad, round_orders=False, fill=0.0):
    K, L = levels.shape
    S, ld = case.prob.S, case.prob.ldb
    ng = L if want_grad else 0
    totals = torch.full((K, 2, S, ld), fill, device=levels.device)
    part = torch.zeros(K, _lib.lib().nic_closed_form_num_partials(case.B, S), ng + 2, device=levels.device)
    _lib.check(_lib.lib().nic_closed_form_sweep(case.desc(levels[0], round_orders), levels.data_ptr(), K, totals.data_ptr(),
                                                part.data_ptr(), ng + 2, int(want_grad), _lib.current_stream()))
    torch.cuda.synchronize()
    return totals, part


def assert_sweep_equals_singles(case, levels, sweep, single):
    """`sweep(levels, want_grad)` / `single(k, want_grad)` (a single-candidate run with levels[k]) -> (totals, second output): every
    candidate's outputs are torch.equal to the single-candidate run's, with and without tangents, and the forward-only values
    equal the with-gradient ones."""
    with_g, without_g = sweep(levels, True), sweep(levels, False)
    assert torch.equal(with_g[0], without_g[0])
    for k in range(levels.shape[0]):
        for got, want_grad in ((with_g, True), (without_g, False)):
            ref = single(k, want_grad)
            assert torch.equal(got[0][k], ref[0]), (k, want_grad)
            if ref[1] is not None:
                assert torch.equal(got[1][k], ref[1]), (k, want_grad)
    return with_g
