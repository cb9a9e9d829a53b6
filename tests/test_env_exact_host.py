"""The exact-input table of tests/env_exact_cases.py through the HOST build of the kernel bodies (tests/hostsim, g++): one period
of dynamics must equal the oracle bit for bit - next state, reward, state and order gradients - at the shapes the fixtures do not
reach (more than 3 warehouses, more than 7 slots, more than 48 scenarios, 1 and 3 echelons).  CPU only; the same table runs through
the HIP library in test_gpu_kernels.py, where the device wrappers are what is on trial."""
import pytest

import env_exact_cases as ex
import kernel_checks as kc


@pytest.fixture(scope="module")
def be():
    return kc.HostSimBackend()


@pytest.mark.parametrize("case", ex.ENV_EXACT_CASES, ids=ex.ENV_EXACT_IDS)
def test_env_step_equals_the_oracle_bit_for_bit(be, case):
    ex.check_env_exact(be, case, in_place=case.in_place, null_grads=case.null_grads)


def test_the_table_reaches_every_instantiation_and_every_planted_tie():
    """The generator really plants what it promises (summed over the table, and each tie on a many-warehouse case of its own), and
    the table launches each of the three slot instantiations."""
    assert {ex.expected_variant(c) for c in ex.ENV_EXACT_CASES} == {4, 8, 16}
    seen = {}
    for c in ex.ENV_EXACT_CASES:
        k, _ = ex.reference(c, c.null_grads)
        for name, hit in ex.planted(k).items():
            seen[name] = seen.get(name, 0) + int(hit)
        if c.S * max(c.Wn, 1) >= 16 and c.B >= 63:
            missing = [n for n, hit in ex.planted(k).items() if not hit]
            assert not missing, (c.id, missing)
    assert all(n > 0 for n in seen.values()), seen
    assert set(seen) == {"on_hand_eq_demand", "zero_store_order", "lead_1", "lead_last_slot", "zero_lead_with_order",
                         "wh_exactly_empty", "wh_short", "wh_left", "zero_wh_order", "zero_ech_order"}


@pytest.mark.parametrize("case", [c for c in ex.ENV_EXACT_CASES if c.id in ("Wn4", "Wn9", "Wn32", "profit-Wn5")], ids=lambda c: c.id)
def test_one_store_bodies_equal_the_quad_composition_beyond_three_warehouses(be, case):
    """The `_t` twins the whole-horizon kernels use have their own "suppliers beyond kSupBatch" loops: composed per store they must
    equal the quad composition bit for bit at Wn = 4, 9 and 32 (the fixtures stop at 3), and under profit with on-hand == demand ties."""
    ex.check_per_store_composition(be.h, case)
