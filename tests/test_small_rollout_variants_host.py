"""csrc/small_rollout_variants.h - which instantiation of the whole-horizon small-rollout kernels a request runs and the name recorded
for it - through the stand-alone host program of tests/test_small_ensemble_host.py.  The expected values are written out HERE, cell by
cell; nothing below is computed through the header."""
import pytest

from test_small_ensemble_host import harness  # noqa: F401  (the module-scoped fixture that builds tests/small_ensemble_plan_harness.cpp)

ROUTES = {"fwd": 0, "wgrad": 1, "dz": 2}
SHAPES = {"any": 0, "one_store": 1, "serial": 2}

# route, chain shape, n_hidden -> the instantiation <NL, SHAPE>.  The forward and the backward with in-kernel weight gradients compile
# both shipped chains in at two and three hidden layers; the dz-history backward only (one_store, 3) and (serial, 2): its (one_store, 2)
# and (serial, 3) run the run-time-structure kernel.
INSTANTIATION = """
fwd    any        1   1 any
fwd    any        2   2 any
fwd    any        3   3 any
fwd    one_store  1   1 any
fwd    one_store  2   2 one_store
fwd    one_store  3   3 one_store
fwd    serial     1   1 any
fwd    serial     2   2 serial
fwd    serial     3   3 serial
wgrad  any        1   1 any
wgrad  any        2   2 any
wgrad  any        3   3 any
wgrad  one_store  1   1 any
wgrad  one_store  2   2 one_store
wgrad  one_store  3   3 one_store
wgrad  serial     1   1 any
wgrad  serial     2   2 serial
wgrad  serial     3   3 serial
dz     any        1   1 any
dz     any        2   2 any
dz     any        3   3 any
dz     one_store  1   1 any
dz     one_store  2   2 any
dz     one_store  3   3 one_store
dz     serial     1   1 any
dz     serial     2   2 serial
dz     serial     3   3 any
"""
CELLS = [(r, s, int(n), int(nl), inst) for r, s, n, nl, inst in (line.split() for line in INSTANTIATION.strip().splitlines())]
# the kernel of a (route, scenarios per wavefront); the dz-history route has no 16-wide form
STEM = {("fwd", 32): "small_rollout_fwd_mfma_kernel", ("fwd", 16): "small_rollout16_fwd_kernel",
        ("wgrad", 32): "small_rollout_bwd_mfma_kernel", ("wgrad", 16): "small_rollout16_bwd_kernel",
        ("dz", 32): "small_rollout_bwd_mfma_kernel"}
NAMES = [  # (route, width, n_hidden, shape, models) -> the recorded name, spelled out
    (("fwd", 32, 3, "one_store", 0), "small_rollout_fwd_mfma_kernel<3,one_store>"),
    (("wgrad", 32, 2, "serial", 3), "small_rollout_bwd_mfma_kernel<2,wgrad,serial,models=3>"),
    (("dz", 32, 3, "any", 0), "small_rollout_bwd_mfma_kernel<3,any>"),
    (("wgrad", 16, 1, "any", 0), "small_rollout16_bwd_kernel<1,wgrad,any>"),
    (("fwd", 16, 2, "serial", 3), "small_rollout16_fwd_kernel<2,serial,models=3>"),
    (("fwd", 32, 1, "any", 65535), "small_rollout_fwd_mfma_kernel<1,any,models=65535>"),
    (("wgrad", 16, 3, "one_store", 1), "small_rollout16_bwd_kernel<3,wgrad,one_store,models=1>"),
    # the recorded name states the request: the two dz-history cells without a kernel of their own keep their shape's name
    (("dz", 32, 2, "one_store", 0), "small_rollout_bwd_mfma_kernel<2,one_store>"),
    (("dz", 32, 3, "serial", 0), "small_rollout_bwd_mfma_kernel<3,serial>"),
]


def test_the_table_covers_every_admitted_cell_once():
    assert len(CELLS) == len({c[:3] for c in CELLS}) == 27
    assert {c[:3] for c in CELLS} == {(r, s, n) for r in ROUTES for s in SHAPES for n in (1, 2, 3)}
    assert sorted(c[:3] for c in CELLS if c[0] == "dz" and c[1] != "any" and c[2] > 1 and c[4] == "any") == [
        ("dz", "one_store", 2), ("dz", "serial", 3)]


@pytest.mark.parametrize("route,shape,n_hidden,nl,inst", CELLS)
def test_variant_and_dispatch_of_every_cell(harness, route, shape, n_hidden, nl, inst):  # noqa: F811
    assert harness("variant", ROUTES[route], SHAPES[shape], n_hidden) == f"{nl} {inst}"
    # the dispatcher hands its callable those constants: one model, and K models where the route has an ensemble form
    assert harness("dispatch", ROUTES[route], SHAPES[shape], n_hidden, 0) == f"{nl} {SHAPES[inst]} 0"
    want = "none" if route == "dz" else f"{nl} {SHAPES[inst]} 1"
    assert harness("dispatch", ROUTES[route], SHAPES[shape], n_hidden, 1) == want


@pytest.mark.parametrize("route,shape,n_hidden,nl,inst", CELLS)
def test_recorded_name_of_every_cell_width_and_model_count(harness, route, shape, n_hidden, nl, inst):  # noqa: F811
    for width in (16, 32):
        if (route, width) not in STEM:   # no 16-wide dz-history kernel: nic_small_rollout_bwd refuses lane_scenarios = 16
            continue
        tag = "wgrad," if route == "wgrad" else ""
        for models in ((0,) if route == "dz" else (0, 3)):   # ... and no ensemble form
            tail = f",models={models}" if models else ""
            assert harness("name", ROUTES[route], width, n_hidden, SHAPES[shape], models) == \
                f"{STEM[route, width]}<{n_hidden},{tag}{shape}{tail}>"


@pytest.mark.parametrize("args,name", NAMES)
def test_recorded_names_spelled_out(harness, args, name):  # noqa: F811
    route, width, n_hidden, shape, models = args
    assert harness("name", ROUTES[route], width, n_hidden, SHAPES[shape], models) == name


def test_no_kernel_outside_one_to_three_hidden_layers(harness):  # noqa: F811
    for route in ROUTES.values():
        for n_hidden in (0, 4):
            assert harness("dispatch", route, 0, n_hidden, 0) == "none"


def test_shape_classifier_and_lane_width(harness):  # noqa: F811
    # Ws Wn Ww E We head F n_out lane_scenarios
    assert harness("classify", 4, 0, 0, 0, 0, 0, 4, 1, 0) == "one_store 32"
    assert harness("classify", 4, 0, 7, 0, 9, 0, 4, 1, 16) == "one_store 16"    # (Ww / We mean nothing without warehouse / echelons)
    assert harness("classify", 4, 1, 3, 2, 4, 1, 15, 4, 32) == "serial 32"
    assert harness("classify", 3, 0, 0, 0, 0, 0, 3, 1, 16) == "any 16"          # a 3-slot store
    assert harness("classify", 4, 1, 3, 1, 4, 1, 11, 3, 0) == "any 32"          # one echelon
    assert harness("classify", 4, 1, 4, 2, 4, 1, 16, 4, 16) == "any 16"         # a 4-slot warehouse
    assert harness("classify", 4, 1, 3, 2, 4, 0, 15, 4, 0) == "any 32"          # the serial chain under the other head
