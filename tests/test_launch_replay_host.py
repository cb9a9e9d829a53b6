"""Host tests of the launch-mode state machine both rollout engines share (`launch_replay.LaunchReplay`) and of the
observation-row filler of the data_driven policy (`layout.fill_observation_rows`).  No GPU: torch.cuda's graph, event and
synchronisation entry points are replaced by recording fakes."""
import pytest
import torch

from neural_inventory_control_amd import launch_replay, layout
from neural_inventory_control_amd.launch_replay import LaunchReplay


class _Log:
    def __init__(self):
        self.captures, self.replays, self.syncs, self.events, self.gpu_ms = 0, 0, 0, 0, 10.0


@pytest.fixture
def cuda(monkeypatch):
    log = _Log()

    class Graph:
        def replay(self):
            log.replays += 1

    class Capture:
        def __init__(self, g):
            assert isinstance(g, Graph)

        def __enter__(self):
            log.captures += 1

        def __exit__(self, *exc):
            return False

    class Event:
        def __init__(self, enable_timing=False):
            assert enable_timing
            log.events += 1

        def record(self):
            pass

        def synchronize(self):
            log.syncs += 1

        def elapsed_time(self, other):
            return log.gpu_ms

    def synchronize():
        log.syncs += 1
    monkeypatch.setattr(torch.cuda, "CUDAGraph", Graph)
    monkeypatch.setattr(torch.cuda, "graph", Capture)
    monkeypatch.setattr(torch.cuda, "Event", Event)
    monkeypatch.setattr(torch.cuda, "synchronize", synchronize)
    return log


class _Launches:
    """A launch sequence: counts how often the host ran it (eagerly or under capture)."""

    def __init__(self):
        self.n = 0

    def __call__(self):
        self.n += 1


def _run(lr, fns, timer=None):
    """One training run of an engine as far as the launch mode sees it."""
    for key, fn in fns.items():
        lr.call(key, fn, timer)
    lr.ran()


def test_first_call_is_eager_second_captures_once_per_key_then_replays(cuda):
    lr = LaunchReplay()
    lr.use_graph = True
    fns = {"fwd": _Launches(), ("bwd", 3): _Launches()}
    _run(lr, fns)
    assert (cuda.captures, cuda.replays, cuda.syncs) == (0, 0, 0) and [f.n for f in fns.values()] == [1, 1] and not lr.graphs
    _run(lr, fns)   # captured (the host runs the sequence once more, under capture) and replayed
    assert (cuda.captures, cuda.replays) == (2, 2) and [f.n for f in fns.values()] == [2, 2]
    assert cuda.syncs == 2   # one synchronisation in front of every capture
    assert set(lr.graphs) == set(fns)
    for _ in range(3):
        _run(lr, fns)
    assert (cuda.captures, cuda.replays, cuda.syncs) == (2, 8, 2) and [f.n for f in fns.values()] == [2, 2]


def test_replay_off_and_timer_force_eager_launches(cuda):
    lr = LaunchReplay()
    fns = {"fwd": _Launches()}
    for _ in range(3):   # use_graph False (the default)
        _run(lr, fns)
    assert (cuda.captures, cuda.replays, fns["fwd"].n) == (0, 0, 3) and not lr.on()
    lr.use_graph = True
    for _ in range(3):
        _run(lr, fns, timer=object())
    assert (cuda.captures, cuda.replays, fns["fwd"].n) == (0, 0, 6) and not lr.graphs
    _run(lr, fns)   # (the timed runs counted as runs: the next one without a timer captures)
    assert (cuda.captures, cuda.replays) == (1, 1)


class _Prob:
    def __init__(self, layout_id):
        self.layout_id, self.refreshed_from = layout_id, []

    def same_layout(self, other):
        return self.layout_id == other.layout_id

    def copy_tables_from(self, other):
        self.refreshed_from.append(other)


def _captured(cuda):
    lr = LaunchReplay()
    lr.use_graph = True
    fns = {"fwd": _Launches(), "bwd": _Launches()}
    p0, d0 = _Prob(0), torch.arange(24.0).view(3, 2, 4)
    for _ in range(2):
        assert lr.pin_problem(p0) is p0
        lr.stage_demand(d0)
        lr.set_variant(("rule", 0))
        _run(lr, fns)
    assert set(lr.graphs) == {"fwd", "bwd"} and cuda.captures == 2
    return lr, fns, p0, d0


def _back_to_one_eager_run(lr, fns, cuda):
    assert not lr.graphs and lr.eager_runs == 0
    captures, replays, n = cuda.captures, cuda.replays, fns["fwd"].n
    _run(lr, fns)
    assert (cuda.captures, cuda.replays, fns["fwd"].n) == (captures, replays, n + 1)   # eager
    _run(lr, fns)
    assert (cuda.captures, cuda.replays) == (captures + 2, replays + 2) and set(lr.graphs) == {"fwd", "bwd"}


def test_a_new_variant_drops_the_captures(cuda):
    lr, fns, _, _ = _captured(cuda)
    assert lr.set_variant(("rule", 0)) is False and len(lr.graphs) == 2
    assert lr.set_variant(("rule", 1)) is True
    _back_to_one_eager_run(lr, fns, cuda)


def test_the_first_variant_is_reported_and_costs_no_run(cuda):
    lr = LaunchReplay()
    lr.use_graph = True
    lr.ran()
    assert lr.set_variant(("rule", 0)) is True and lr.eager_runs == 1


def test_a_demand_shape_change_drops_the_captures(cuda):
    lr, fns, _, d0 = _captured(cuda)
    buf = lr.stage_demand(d0)
    assert len(lr.graphs) == 2 and torch.equal(buf, d0) and buf.data_ptr() != d0.data_ptr()
    d1 = torch.ones(4, 2, 4)
    buf1 = lr.stage_demand(d1)
    assert buf1.shape == d1.shape and torch.equal(buf1, d1) and buf1.data_ptr() != d1.data_ptr()
    _back_to_one_eager_run(lr, fns, cuda)


def test_a_problem_of_another_layout_is_pinned_and_drops_the_captures(cuda):
    lr, fns, p0, _ = _captured(cuda)
    same = _Prob(0)
    assert lr.pin_problem(same) is p0 and p0.refreshed_from[-1] is same and len(lr.graphs) == 2   # tables refreshed in place
    other = _Prob(1)
    assert lr.pin_problem(other) is other and other.refreshed_from == []
    _back_to_one_eager_run(lr, fns, cuda)
    assert lr.pin_problem(_Prob(1)) is other


def test_stage_demand_skips_the_copy_when_handed_its_own_buffer(cuda, monkeypatch):
    lr = LaunchReplay()
    d = torch.arange(24.0).view(3, 2, 4)
    assert lr.stage_demand(d) is d and lr.pin_problem("p") == "p" and lr.demand is None   # eager launches: passed through
    lr.use_graph = True
    buf = lr.stage_demand(d)
    copies = []
    real = torch.Tensor.copy_
    monkeypatch.setattr(torch.Tensor, "copy_", lambda self, src, *a, **k: (copies.append(src), real(self, src, *a, **k))[1])
    assert lr.stage_demand(buf) is buf and copies == []
    assert lr.stage_demand(d + 1) is buf and len(copies) == 1 and torch.equal(buf, d + 1)


@pytest.mark.parametrize("host_ms, gpu_ms", [(9.0, 10.0), (8.0, 10.0), (8.5, 10.0), (0.2, 0.1)])
def test_probe_publishes_the_rule_and_runs_once_after_an_eager_training_run(cuda, monkeypatch, host_ms, gpu_ms):
    cuda.gpu_ms = gpu_ms
    clock = iter([100.0, 100.0 + host_ms / 1e3])
    monkeypatch.setattr(launch_replay.time, "perf_counter", lambda: next(clock))
    lr = LaunchReplay()
    lr.use_graph = "auto"

    def run(train, timer=None):
        lr.probe_begin(train, timer)
        lr.call("fwd", lambda: None, timer)
        if train:
            lr.probe_end()
        lr.ran()
    run(True)                    # no eager run before it: not measured
    assert lr.probe is None and cuda.events == 0
    run(False)                   # an evaluation run counts as a run and is not measured
    assert lr.probe is None and lr.eager_runs == 2 and cuda.events == 0
    run(True, timer=object())    # a timer: not measured
    assert lr.probe is None and cuda.events == 0 and not lr.on()
    run(True)
    p = lr.probe
    assert p["gpu_ms"] == gpu_ms and abs(p["host_enqueue_ms"] - host_ms) < 1e-6
    assert p["replay"] == (p["host_enqueue_ms"] > 0.85 * p["gpu_ms"]) == lr.on() == lr.decision
    assert cuda.events == 2 and cuda.captures == 0
    run(True)                    # decided: not measured again (the clock has no third reading)
    assert cuda.events == 2 and lr.probe is p and cuda.captures == (1 if p["replay"] else 0)


def test_reset_forgets_the_decision_the_captures_and_the_buffers(cuda):
    lr, fns, p0, d0 = _captured(cuda)
    lr.use_graph, lr.decision = "auto", True
    assert lr.on()
    lr.reset(buffers=False)      # GnnRollout's: the staging buffer and the pinned problem stay
    assert not lr.on() and lr.decision is None and not lr.graphs and lr.eager_runs == 0
    assert lr.demand is not None and lr.prob is p0
    lr.decision = True
    lr.reset()
    assert not lr.on() and lr.decision is None and lr.demand is None and lr.prob is None
    lr.use_graph = True
    lr.invalidate()
    assert lr.on() and not lr.graphs and lr.eager_runs == 0


def test_engines_serve_the_names_tools_read_from_their_launch_replay():
    from neural_inventory_control_amd.gnn_rollout import GnnRollout
    from neural_inventory_control_amd.rollout import FusedRollout
    for cls in (FusedRollout, GnnRollout):
        eng = cls.__new__(cls)
        eng._replay = LaunchReplay()
        assert eng.use_graph is False and eng._graphs == {} and eng.auto_graph_probe is None and not eng._graph_on()
        eng.use_graph = True
        assert eng._replay.use_graph is True and eng._graph_on()
        eng._replay.graphs["fwd"] = object()
        assert set(eng._graphs) == {"fwd"}


# ---- observation rows of the data_driven policy ---------------------------------------------------------------------------------
S, P, T, B, LD, D, W, F_DYN = 2, 3, 4, 5, 32, 1, 1, 3
N_T, N_DFC = T + 2, 5
F = F_DYN + S * P + 2 * S + D + S * W
UNTOUCHED = -7.0


def _observation_case():
    g = torch.Generator().manual_seed(3)
    r = lambda *s: torch.rand(*s, generator=g) + 0.5  # noqa: E731
    data = {"demands": r(B, S, N_T), "underage_costs": r(B, S), "holding_costs": r(B, S), "days_from_christmas": r(B, D, N_DFC),
            "lead_times": r(B, S, W)}
    return data, layout.demand_trace_soa(data["demands"], LD)


def _expected_blocks(data, shift):
    """[T][F][ld] by the reference's rules, one period and one row at a time: the window of the P demands before period
    t + shift (zeros to the left of period 0), underage and holding costs, the days-from-christmas column of period t + shift
    (the last one beyond the data), lead times; in the policy's concatenation order.  Only the first B columns of the per-scenario
    rows are written; state rows are not touched."""
    X = torch.full((T, F, LD), UNTOUCHED)
    for t in range(T):
        now, o = t + shift, F_DYN
        for s in range(S):
            for p in range(P):
                period = now - P + p
                X[t, o, :] = 0.0
                if period >= 0:
                    X[t, o, :B] = data["demands"][:, s, period]
                o += 1
        for k in ("underage_costs", "holding_costs"):
            for s in range(S):
                X[t, o, :B] = data[k][:, s]
                o += 1
        for d in range(D):
            X[t, o, :B] = data["days_from_christmas"][:, d, min(now, N_DFC - 1)]
            o += 1
        for s in range(S):
            for w in range(W):
                X[t, o, :B] = data["lead_times"][:, s, w]
                o += 1
        assert o == F
    return X


@pytest.mark.parametrize("shift", [0, 2])
def test_observation_rows_equal_a_per_period_loop_in_both_block_orders(shift):
    data, demand_soa = _observation_case()
    want = _expected_blocks(data, shift)
    X = torch.full((T + 1, F + 1, LD), UNTOUCHED)   # (the per-period route's blocks: one more period, one more row)
    end = layout.fill_observation_rows(X[:T], F_DYN, S, P, T, B, shift, data, demand_soa, torch.zeros(P + N_T, S, LD))
    assert end == F
    assert torch.equal(X[:T, :F], want)
    assert bool((X[T] == UNTOUCHED).all()) and bool((X[:, F] == UNTOUCHED).all())
    by_row = torch.full((F, T, LD), UNTOUCHED)      # the whole-horizon route's [F][T][ld]
    assert layout.fill_observation_rows(by_row.transpose(0, 1), F_DYN, S, P, T, B, shift, data, demand_soa,
                                        torch.zeros(P + N_T, S, LD)) == F
    assert torch.equal(by_row, want.transpose(0, 1))
    assert torch.equal(by_row, X[:T, :F].transpose(0, 1))
