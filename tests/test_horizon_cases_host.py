"""Conditions on the inputs of tests/horizon_cases.py, asserted from the float64 / float32 reference alone (no kernel, no GPU): the
table is only a referee for csrc/horizon_rollout.hip if few scenarios sit on a knife edge, both sides of every decision occur, the
float32 run stays inside the decision margin, and the shapes launch every instantiation."""
import pytest
import torch

import horizon_cases as hc


@pytest.mark.parametrize("c", hc.ALL_CASES, ids=hc.CASE_IDS)
def test_horizon_case_conditions(c):
    r64, r32 = hc.reference(c, torch.float64), hc.reference(c, torch.float32)
    s = r64["stats"]
    excluded = int((~hc.kept(c)).sum())
    print(f"{c.id}: excluded {excluded} of {c.B}; smallest margin by decision "
          + ", ".join(f"{k} {float(v.min()):.1e}" for k, v in r64["margins"].items()) + f"; {s}")
    assert excluded <= hc.MAX_EXCLUDED * c.B
    if c.mode == 0:
        assert s["logit_pos"] > 0 and s["logit_neg"] > 0
        if c.Wn >= 2:
            assert s["bind"] > 0 and s["free"] > 0
    if c.mode == 2 and not c.allow_negative:
        assert s["clip_on"] > 0 and s["clip_off"] > 0
    # the float32 run of the reference against the float64 run: its own rounding, the yardstick of the kernels' bar.  It has to stay
    # inside the decision margin, or the two runs would not be on the same branches of the kept scenarios.
    e32 = hc.yardstick(c)
    print(f"{c.id}: worst-row e32 " + ", ".join(f"{n} {v:.1e}" for n, v in e32.items()))
    for n, v in e32.items():
        assert v < hc.KNIFE_EDGE, (c.id, n, v)
    for n in hc.GRAD_QUANTITIES:
        if n in r64:
            assert r64[n].shape == r32[n].shape
            if c.id != "min":
                assert float(r64[n][..., hc.kept(c)].abs().max()) > 0, (c.id, n, "no gradient to compare")


def test_horizon_allocation_branches_across_one_warehouse_cases():
    one = [hc.reference(c, torch.float64)["stats"] for c in hc.HORIZON_CASES if c.Wn == 1]
    assert len(one) >= 2 and sum(s["bind"] for s in one) > 0 and sum(s["free"] for s in one) > 0


def test_horizon_table_launches_every_instantiation():
    names = set()
    for c in hc.HORIZON_CASES:
        names.update(hc.expected_kernels(c))
    assert names == hc.ALL_KERNELS
    # both sides of every threshold of fwd_steps (64, 160) and bwd_variant (FD 64 / 192, n_out 16 / 80)
    dims = [hc.dims_of(c)[:2] for c in hc.HORIZON_CASES]
    for fd in (64, 65, 160, 161, 256):
        assert any(d[0] == fd for d in dims), fd
    for n_out in (16, 80, 81, 128):
        assert any(d[1] == n_out for d in dims), n_out
    assert any(d[0] <= 64 and d[1] > 80 for d in dims)     # forward <8,16> under backward <8,2>
    assert any(192 < d[0] for d in dims) and any(160 < d[0] <= 192 or d[0] == 200 for d in dims)


def test_horizon_table_varies_the_launch_parameters():
    cs = hc.ALL_CASES
    assert {c.B for c in cs} >= {1, 16, 17, 33, 40} and {c.T for c in cs} >= {3, 4, 5} and {c.t0 for c in cs} == {0, 2}
    assert any(c.ldb == -(-c.B // 16) * 16 for c in cs) and any(c.ldb > -(-c.B // 16) * 16 for c in cs)
    assert any(c.hist_gap for c in cs) and any(not c.hist_gap for c in cs) and any(c.w_gap for c in cs)
    for flag in ("per_scenario", "g_uniform", "profit", "lost", "edge"):
        assert {bool(getattr(c, flag)) for c in hc.HORIZON_CASES} == {False, True}, flag
