"""The sweep chain of closed_form_body.h (KC candidate level vectors per lane against one fetched demand value) compiled for the
host: every candidate's per-chain totals, reported costs and level gradients EQUAL those of the single-candidate chain run with
that candidate's levels, for every group size, including a ragged last group."""
import functools

import pytest
import torch

import closed_form_checks as cfc
import closed_form_sweep_checks as swc
import hostsim_sweep_util
import hostsim_util


@functools.lru_cache(maxsize=None)
def _golden(name):
    """(case, candidates [5][L], single-candidate references per row: with and without tangents) - computed once per case"""
    case = swc.golden_case(name, "cpu")
    levels = case.candidates(swc.SCALES_5)
    return case, levels, _singles(case, levels)


@functools.lru_cache(maxsize=None)
def _serial(seed):
    case = swc.serial_case(seed, "cpu")
    levels = case.candidates((0.7, 1.0, 1.4))
    return case, levels, _singles(case, levels)


def _singles(case, levels):
    h = hostsim_util.load()
    return {(k, wg): swc.host_single(h, case, levels[k].contiguous(), wg) for k in range(levels.shape[0]) for wg in (True, False)}


def _check(case, levels, refs, kc):
    hs = hostsim_sweep_util.load()
    swc.assert_sweep_equals_singles(case, levels, lambda lv, wg: swc.host_sweep(hs, case, lv, kc, wg), lambda k, wg: refs[(k, wg)])


@pytest.mark.parametrize("kc", [1, 2, 4])
@pytest.mark.parametrize("name", cfc.CLOSED_FORM_CASES)
def test_sweep_chain_equals_single_candidate_chain_on_golden_cases(name, kc):
    """K = 5 (the fixture's levels in row 2, the others scaled by 0.5 / 0.8 / 1.3 / 2.0): a ragged last group for KC = 2 and 4."""
    case, levels, refs = _golden(name)
    _check(case, levels, refs, kc)


@pytest.mark.parametrize("kc", [1, 2, 4])
@pytest.mark.parametrize("name", cfc.CLOSED_FORM_CASES)
def test_sweep_row_with_the_fixture_levels_reproduces_the_golden_costs(name, kc):
    case, levels, _ = _golden(name)
    totals, _ = swc.host_sweep(hostsim_sweep_util.load(), case, levels, kc, True)
    g = case.golden
    total, reported = float(totals[2, 0].double().sum()), float(totals[2, 1].double().sum())
    assert abs(total - float(g.z["total"])) <= 1e-6 * abs(float(g.z["total"]))
    assert abs(reported - float(g.z["reported"])) <= 1e-6 * abs(float(g.z["reported"]))


@pytest.mark.parametrize("kc", [1, 2, 4])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_sweep_chain_equals_single_candidate_chain_on_random_serial_systems(seed, kc):
    """n = 70 / 128 / 200 chains, T off the 8-period fetch batch, 1-3 extra echelons, K = 3."""
    case, levels, refs = _serial(seed)
    _check(case, levels, refs, kc)
