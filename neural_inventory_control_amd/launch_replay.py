"""`LaunchReplay`: the launch-mode state of a rollout engine (`FusedRollout`, `GnnRollout`), in one place.

The launch sequence of a rollout is identical from call to call (same buffers, same shapes), so after one eager run (module
loading is not capturable) it can be captured into HIP graphs and replayed, which removes the per-launch host cost that bounds
the small batches.  `use_graph` is True / False, or "auto" = decided by MEASUREMENT on the second training run of a shape: if
the host needs longer to enqueue the step than the GPU needs to run it, the step is launch-bound and later runs are replayed.

A capture holds raw pointers, so what it reads must stay where it is: the demand trace is staged in a buffer owned here, and
the first run's `EnvProblem` is pinned and its tables refreshed in place.  Whatever else is baked into a capture is the
engine's `variant`; a change of any of these drops the captures.
"""
import time

import torch

_NO_VARIANT = object()


class LaunchReplay:
    def __init__(self):
        self.use_graph = False
        self.graphs = {}        # key -> torch.cuda.CUDAGraph (HIP graph) of one launch sequence
        self.eager_runs = 0     # runs since the captures were last dropped (the first one is never captured)
        self.decision = None    # "auto": None = not measured yet, else whether to replay
        self.probe = None       # what "auto" measured (the engines' `auto_graph_probe`)
        self.demand = None      # staging buffer of the demand trace
        self.prob = None        # pinned EnvProblem
        self.variant = _NO_VARIANT   # what the engine says its captures were taken under
        self._probing = None

    def on(self):
        return self.use_graph is True or (self.use_graph == "auto" and self.decision is True)

    def invalidate(self):
        self.graphs, self.eager_runs = {}, 0

    def reset(self, buffers=True):
        """A new shape: measured afresh; `buffers`: the staging buffer and the pinned problem go too."""
        self.invalidate()
        self.decision = None
        if buffers:
            self.demand = self.prob = None

    def stage_demand(self, demand_soa):
        """The trace a launch sequence reads: the caller's while launches are eager, else this object's copy of it."""
        if not self.on():
            return demand_soa
        if self.demand is None or self.demand.shape != demand_soa.shape:
            self.demand = torch.empty_like(demand_soa)
            self.invalidate()
        if self.demand.data_ptr() != demand_soa.data_ptr():
            self.demand.copy_(demand_soa)
        return self.demand

    def pin_problem(self, prob):
        """The problem a launch sequence reads: the caller's while launches are eager, else the pinned one, refreshed."""
        if not self.on():
            return prob
        if self.prob is not None and self.prob.same_layout(prob):
            self.prob.copy_tables_from(prob)
        else:
            self.prob = prob
            self.invalidate()
        return self.prob

    def set_variant(self, variant):
        """True if `variant` is not what the last call gave.  Captures taken under another one are dropped (the first variant
        is only recorded: nothing was captured before it)."""
        changed = variant != self.variant
        if changed and self.variant is not _NO_VARIANT:
            self.invalidate()
        self.variant = variant
        return changed

    def call(self, key, fn, timer=None):
        """Runs `fn`'s launches: eagerly (replay off, a timer attached, or the first run), else from the capture under `key`,
        taken now if there is none."""
        if not self.on() or timer is not None or self.eager_runs < 1:
            return fn()
        g = self.graphs.get(key)
        if g is None:
            g = torch.cuda.CUDAGraph()
            torch.cuda.synchronize()
            with torch.cuda.graph(g):
                fn()
            self.graphs[key] = g
        g.replay()

    def ran(self):
        self.eager_runs += 1

    def probe_begin(self, train, timer=None):
        """"auto", once per shape: brackets a training run that follows an eager one (no timer) for `probe_end`."""
        self._probing = None
        if self.use_graph == "auto" and self.decision is None and train and self.eager_runs >= 1 and timer is None:
            ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            torch.cuda.synchronize()
            ev[0].record()
            self._probing = (ev, time.perf_counter())

    def probe_end(self):
        """Host time to enqueue the step against GPU time to run it (one synchronisation)."""
        if self._probing is None:
            return
        ev, t0 = self._probing
        self._probing = None
        host_ms = (time.perf_counter() - t0) * 1e3
        ev[1].record()
        ev[1].synchronize()
        gpu_ms = ev[0].elapsed_time(ev[1])
        self.decision = host_ms > 0.85 * gpu_ms
        self.probe = {"host_enqueue_ms": host_ms, "gpu_ms": gpu_ms, "replay": self.decision}


class ReplayedEngine:
    """What tests, tools and bench.py read and set on an engine, served by its `LaunchReplay` (`self._replay`)."""
    use_graph = property(lambda self: self._replay.use_graph, lambda self, v: setattr(self._replay, "use_graph", v))
    _graphs = property(lambda self: self._replay.graphs)
    auto_graph_probe = property(lambda self: self._replay.probe)

    def _graph_on(self):
        return self._replay.on()
