"""The mlp3 checker (tests/mlp3_checks.py) checked on the CPU: the clean float32 emulation of the kernels passes every case of the
table, every class of kernel error the emulation can restate (`defect=`) fails at least one, the band's constant follows from the
float32-against-float64 measurement, and the table reaches every dispatch cell of the launchers."""
import re

import pytest
import torch

import mlp3_checks as mc

# cases with thousands of (entity, chunk) items: run under the defects that need that many only
_MANY_ITEMS = [c for c in mc.CASES if c.E_live * ((c.B + 31) // 32) > 2048]


@pytest.mark.parametrize("case", mc.CASES, ids=[c.id for c in mc.CASES])
def test_the_clean_emulation_passes(case):
    figures = mc.check_case(case, mc.EmulatedMlp3())
    assert max(figures.values()) <= 1.0


def test_every_defect_fails_at_least_one_case():
    caught = {d: [] for d in mc.DEFECTS}
    for case in mc.CASES:
        for defect in mc.DEFECTS:
            if case in _MANY_ITEMS and defect != "resets_grads_per_item":
                continue
            try:
                mc.check_case(case, mc.EmulatedMlp3(defect))
            except AssertionError:
                caught[defect].append(case.id)
    for defect, ids in caught.items():
        print(f"{defect}: caught by {len(ids)} cases: {' '.join(ids)}")
    assert all(caught.values()), [d for d, ids in caught.items() if not ids]
    # accumulation across items shows only where a wavefront walks more than one
    assert set(caught["resets_grads_per_item"]) <= {c.id for c in _MANY_ITEMS}


def test_the_band_constant_follows_from_the_float32_measurement():
    """C = max(8 x the largest err / scale plain float32 torch shows against float64 over the table, the GEMM band 4e-6)."""
    worst = {}
    for case in mc.CASES:
        for k, v in mc.problem(case).float32_ratios().items():
            worst[k] = max(worst.get(k, 0.0), v)
    print("float32 against float64, largest err / scale:", "  ".join(f"{k} {v:.1e}" for k, v in worst.items()))
    assert mc.C_BAND == max(4e-6, 8 * mc.F32_WORST)
    # (the summation order of a CPU GEMM depends on the library and its thread count: the recorded figure within a factor 2)
    assert mc.F32_WORST / 2 <= max(worst.values()) <= 2 * mc.F32_WORST, worst


def test_the_table_reaches_every_dispatch_cell():
    names = {n for c in mc.CASES for n in mc.expected_kernels(c)}
    want = {f"mlp3_bwd_hist_kernel<{kg},{mode}{tail}>" for kg in (1, 2, 3) for mode in ("stored", "gather")
            for tail in ("", ",tail") if not (kg == 3 and tail)}
    want |= {f"mlp3_bwd_fused_kernel<{kg}>" for kg in (1, 2, 3)}
    assert want <= names, sorted(want - names)
    fwd = [tuple(map(int, re.findall(r"\d+", n)[1:])) for n in names if n.startswith("mlp3_fwd_kernel")]
    assert {f[0] for f in fwd} == {4, 16, 33, 48} and {f[1] for f in fwd} == {1, 2} and {f[2] for f in fwd} == {1, 2}, fwd
    # ... and the shapes the engine's layouts need: native history under the pair variant, live < held entities with and without
    # the residual, an interleaved period under both input modes, every scenario-count edge, n_out 1..32 under each activation
    has = lambda pred: any(pred(c) for c in mc.CASES)  # noqa: E731
    assert has(lambda c: c.hist == "native" and ",2," in mc.expected_kernels(c)[0] and (mc.pad32(c.B) // 32) % 2 == 1)
    assert has(lambda c: c.E_buf > c.E_live and c.residual) and has(lambda c: c.E_buf > c.E_live and not c.residual)
    assert {c.x_hist for c in mc.CASES if isinstance(c.hist, tuple)} == {"stored", "gather"}
    assert {1, 31, 32, 33, 64, 70} <= {c.B for c in mc.CASES if c.hist == "native"}
    assert {(n, a) for n in (1, 5, 8, 12, 20, 31, 32) for a in (0, 1, 2)} <= {(c.n_out, c.act) for c in mc.CASES}
    assert has(lambda c: len(c.segs) == 4 and sum(s.kind == "map" for s in c.segs) == 2 and c.segs[-1].kind == "const")
    assert has(lambda c: any(s.kind == "bcast" for s in c.segs))


def test_the_un_permute_of_the_native_layout_is_the_documented_one():
    """Block e * ldb / 32 + chunk of the buffer is [32 rows][32 scenarios] of entity e (include/nic_rollout.h), stated with a loop."""
    case = mc.BY_ID["live5of9-edge-native-B70"]
    h = mc.Hist(case, 32, 96, "cpu")
    h.full.copy_(torch.arange(h.full.numel(), dtype=torch.float32).view_as(h.full))
    cur, rest = h.dense()
    blocks = h.full[h.t].view(-1, 32, 32)
    for e in range(case.E_buf):
        for chunk in range(3):
            assert torch.equal(cur[:, e, 32 * chunk:32 * chunk + 32], blocks[e * 3 + chunk])
    assert rest.numel() == 2 * h.full[0].numel()
