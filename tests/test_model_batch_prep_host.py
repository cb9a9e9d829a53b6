"""What every engine does with a model and a batch before it launches anything, as device-free functions: LazyLinear
materialisation, the materialised layers and the order upper bound (policy_layers.py); the initial-state block, the edge mask and
the data_driven input's row count (layout.py).  CPU tensors only."""
import types

import pytest
import torch

from golden_io import Golden
from neural_inventory_control_amd import ensemble_step, layout
from neural_inventory_control_amd.neural_networks import NeuralNetworkCreator
from neural_inventory_control_amd.policy_layers import materialize_linears, materialized_linears, upper_bound

DATA_DRIVEN = ("f4_real_many_warehouses_data_driven", "f4_real_one_store_data_driven")


def _lazy_policy(name):
    g = Golden(name)
    c = g.fresh_config()

    class _Sc:
        problem_params = c["problem_params"]
        store_params = {"demand": {"mean": [5.0]}}
    return NeuralNetworkCreator().create_neural_network(_Sc(), c["nn_params"], device="cpu"), g, c


# ---- materialisation ------------------------------------------------------------------------------------------------------------
def test_a_seeded_lazy_chain_gets_the_weights_of_seeded_linears_built_in_the_same_order():
    lazy = [torch.nn.LazyLinear(8), torch.nn.LazyLinear(4, bias=False), torch.nn.LazyLinear(2)]
    torch.manual_seed(11)
    materialize_linears(lazy, 5)
    torch.manual_seed(11)
    want = [torch.nn.Linear(5, 8), torch.nn.Linear(8, 4, bias=False), torch.nn.Linear(4, 2)]
    for got, ref in zip(lazy, want):
        assert type(got) is torch.nn.Linear and (got.in_features, got.out_features) == (ref.in_features, ref.out_features)
        assert torch.equal(got.weight, ref.weight)
        assert (got.bias is None and ref.bias is None) or torch.equal(got.bias, ref.bias)
    # materialised layers are left alone: no RNG is consumed, no value moves
    before = [lin.weight.clone() for lin in lazy]
    state = torch.get_rng_state()
    materialize_linears(lazy, 5)
    assert torch.equal(torch.get_rng_state(), state) and all(torch.equal(lin.weight, w) for lin, w in zip(lazy, before))


def test_the_data_driven_policys_first_layer_is_a_seeded_linear_bit_for_bit():
    model, g, c = _lazy_policy(DATA_DRIVEN[0])
    F, H1 = g.params["net.master.0.weight"].shape[1], c["nn_params"]["neurons_per_hidden_layer"]["master"][0]
    assert F == 597
    torch.manual_seed(3)
    materialize_linears(model.master_linears(), F)
    torch.manual_seed(3)
    ref = torch.nn.Linear(F, H1)
    first = materialized_linears(model)[0]
    assert torch.equal(first.weight, ref.weight) and torch.equal(first.bias, ref.bias)


def test_a_lazy_layer_loaded_from_a_checkpoint_becomes_the_concrete_class_with_its_width():
    model, g, _ = _lazy_policy(DATA_DRIVEN[0])
    model.load_state_dict(g.params)
    first = model.master_linears()[0]
    assert isinstance(first, torch.nn.LazyLinear) and first.in_features == 0   # (what load_state_dict leaves)
    concrete = first.cls_to_become
    materialize_linears(model.master_linears(), 1)   # (the width comes from the loaded weight, not from the argument)
    first = materialized_linears(model)[0]
    assert type(first) is concrete and not isinstance(first, torch.nn.LazyLinear)
    assert first.in_features == g.params["net.master.0.weight"].shape[1]
    assert torch.equal(first.weight, g.params["net.master.0.weight"])
    assert not hasattr(first, "_initialize_hook") and not hasattr(first, "_load_hook")


def test_an_unmaterialised_model_has_no_materialised_layers():
    model, _, _ = _lazy_policy(DATA_DRIVEN[0])
    with pytest.raises(RuntimeError, match=r"policy has un-materialised LazyLinear layers; call materialize\(\) or run one forward"):
        materialized_linears(model)


# ---- initial state ----------------------------------------------------------------------------------------------------------------
B, LDB = 3, 64
SHAPES = [dict(S=2, Ws=3, Wn=0, Ww=0, E=0, We=0), dict(S=1, Ws=2, Wn=1, Ww=2, E=1, We=2)]


def _batch(shape):
    prob = types.SimpleNamespace(B=B, ldb=LDB, **shape)
    gen = torch.Generator().manual_seed(5)
    data = {"initial_inventories": torch.rand(B, prob.S, prob.Ws, generator=gen)}
    if prob.Wn:
        data["initial_warehouse_inventories"] = torch.rand(B, prob.Wn, prob.Ww, generator=gen)
    if prob.E:
        data["initial_echelon_inventories"] = torch.rand(B, prob.E, prob.We, generator=gen)
    return prob, data, prob.S * prob.Ws + prob.Wn * prob.Ww + prob.E * prob.We


def _check_part(block, row0, src):
    n, w = src.shape[1:]
    for s in range(n):
        for j in range(w):
            for b in range(B):
                assert block[row0 + s * w + j, b] == src[b, s, j]
    return row0 + n * w


@pytest.mark.parametrize("shape", SHAPES, ids=["stores", "serial"])
def test_initial_state_block_is_the_references_concatenation(shape):
    prob, data, rows = _batch(shape)
    block = torch.full((rows + 1, LDB), -7.0)   # (pre-filled, and one row more than the state)
    layout.fill_initial_state(block, prob, data)
    o = _check_part(block, 0, data["initial_inventories"])
    if prob.Wn:
        o = _check_part(block, o, data["initial_warehouse_inventories"])
    if prob.E:
        o = _check_part(block, o, data["initial_echelon_inventories"])
    assert o == rows
    assert bool((block[:, B:] == -7.0).all()) and bool((block[rows:] == -7.0).all())


@pytest.mark.parametrize("shape", SHAPES, ids=["stores", "serial"])
def test_stores_only_fills_the_store_rows_and_the_caller_decides_per_part(shape):
    prob, data, rows = _batch(shape)
    block = torch.full((rows, LDB), -7.0)
    layout.fill_initial_state(block, prob, data, stores_only=True)
    a = _check_part(block, 0, data["initial_inventories"])
    assert bool((block[a:] == -7.0).all()) and bool((block[:, B:] == -7.0).all())
    # `changed`: asked once per part with the part's name, the [n][W][B] view to fill and the batch's own tensor
    asked, block2 = [], torch.full((rows, LDB), -7.0)
    layout.fill_initial_state(block2, prob, data, changed=lambda slot, dst, src: asked.append((slot, tuple(dst.shape), src)) or slot != "store")
    assert [a_[0] for a_ in asked] == ["store"] + ["wh"] * bool(prob.Wn) + ["ech"] * bool(prob.E)
    assert asked[0][1] == (prob.S, prob.Ws, B) and asked[0][2] is data["initial_inventories"]
    assert bool((block2[:a] == -7.0).all())
    if prob.Wn:
        assert _check_part(block2, _check_part(block2, a, data["initial_warehouse_inventories"]), data["initial_echelon_inventories"]) == rows


# ---- edge mask, row count -----------------------------------------------------------------------------------------------------------
def test_edge_mask_is_the_contiguous_float_transpose_of_the_adjacency():
    adj = [[1, 0, 1], [0, 1, 1]]   # [Wn = 2][S = 3]
    mask = layout.edge_mask({"n_warehouses": 2, "warehouse_store_adjacency": adj}, "cpu")
    assert mask.dtype == torch.float32 and mask.shape == (3, 2) and mask.is_contiguous()
    assert torch.equal(mask, torch.tensor(adj, dtype=torch.float32).t())
    assert layout.edge_mask({"n_warehouses": 0}, "cpu") is None


@pytest.mark.parametrize("name", DATA_DRIVEN)
def test_data_driven_row_count_is_the_first_layers_width(name):
    g = Golden(name)
    obs = g.fresh_config()["observation_params"]
    state_rows = sum(g.data[k][0].numel() for k in ("initial_inventories", "initial_warehouse_inventories") if k in g.data)
    assert layout.data_driven_input_rows(state_rows, g.data, obs) == g.params["net.master.0.weight"].shape[1]


# ---- upper bound ------------------------------------------------------------------------------------------------------------------
class _CountedReads(torch.Tensor):
    reads = 0

    @classmethod
    def __torch_function__(cls, func, types_, args=(), kwargs=None):
        if func is torch.Tensor.reshape:   # (how `upper_bound` reads the value)
            cls.reads += 1
        return super().__torch_function__(func, types_, args, kwargs or {})


def test_upper_bound_of_a_float_and_of_a_tensor_and_the_cached_form_reads_once_per_version():
    assert upper_bound(types.SimpleNamespace(warehouse_upper_bound=12.5)) == 12.5
    assert upper_bound(types.SimpleNamespace(warehouse_upper_bound=torch.tensor([12.5]))) == 12.5
    assert upper_bound(types.SimpleNamespace(warehouse_upper_bound=12.5), {}) == 12.5
    ub = torch.tensor([12.5]).as_subclass(_CountedReads)
    model, cache = types.SimpleNamespace(warehouse_upper_bound=ub), {}
    _CountedReads.reads = 0
    assert [upper_bound(model, cache) for _ in range(3)] == [12.5] * 3 and _CountedReads.reads == 1
    ub.fill_(4.0)   # an in-place write: the version moves, the next call reads again - once
    assert [upper_bound(model, cache) for _ in range(3)] == [4.0] * 3 and _CountedReads.reads == 2 and len(cache) == 1
    assert upper_bound(model) == 4.0 and upper_bound(model) == 4.0 and _CountedReads.reads == 4   # (uncached: every call reads)


# ---- instance count -----------------------------------------------------------------------------------------------------------------
def test_the_engines_early_count_check_keeps_its_message_for_no_instances_too():
    assert ensemble_step.instance_replicas(2, 6, "SmallPolicyEnsemble") == 3
    for n in (0, 4):
        with pytest.raises(ValueError, match=f"SmallPolicyEnsemble: {n} problem instances do not divide 6 models"):
            ensemble_step.instance_replicas(n, 6, "SmallPolicyEnsemble")
    with pytest.raises(ValueError, match="SmallPolicyEnsemble needs at least one problem instance"):
        ensemble_step.check_instances([], 6)
