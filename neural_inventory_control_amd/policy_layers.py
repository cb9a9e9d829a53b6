"""What the engines ask of an MLP policy model before anything is launched, as functions on the model (no device, no engine): the
policies the MLP engines take, LazyLinear materialisation, the materialised master layers, the scalar order upper bound.
`FusedRollout` (whose `supports` / `observation_ok` / `materialize` are these), `GnnRollout` and the K-model engines call them."""
import torch

HEADS = {"vanilla_one_store": "softplus", "vanilla_warehouse": "warehouse", "vanilla_serial": "serial",
         "data_driven": "data_driven"}


def supports(model):
    name = getattr(model, "nn_args", {}).get("name") if hasattr(model, "nn_args") else None
    if name not in HEADS or type(model).__name__ not in ("VanillaOneStore", "VanillaWarehouse", "VanillaSerial",
                                                         "DataDrivenNet"):
        return False
    a = model.nn_args
    if name == "data_driven":   # the real-data policy (data_driven_net.yml): ELU inside, ReLU on the output layer
        return (type(model).__name__ == "DataDrivenNet" and a["inner_layer_activations"]["master"] == "elu"
                and a["output_layer_activation"]["master"] == "relu" and len(a["neurons_per_hidden_layer"]["master"]) >= 1)
    return (type(model).__name__ != "DataDrivenNet" and a["inner_layer_activations"]["master"] == "elu"
            and a["output_layer_activation"]["master"] is None and len(a["neurons_per_hidden_layer"]["master"]) >= 1)


def observation_ok(model, observation_params, data=None):
    """Can the MLP engine build the policy's observation?  The vanilla policies read the inventories only (no past-demand
    window, no time / sample features: trainer.py's generic loop otherwise); data_driven reads the past-demand window and
    `days_from_christmas` (neural_networks.py:452-470) and nothing else that moves with the period."""
    op = observation_params
    if op is None:
        return False
    past, tf, sf = (op["demand"] or {}).get("past_periods"), op["time_features"], op["sample_features"]
    past = past if isinstance(past, int) else 0   # (`past_periods: null` / a missing key: no window -> the generic route)
    if getattr(model, "nn_args", {}).get("name") == "data_driven":
        # (sample features, e.g. `store_nbr`, may be in the observation: DataDrivenNet.forward does not read them)
        return (isinstance(tf, (list, tuple)) and list(tf) == ["days_from_christmas"] and past >= 1
                and (data is None or ("days_from_christmas" in data and "underage_costs" in data)))
    return past == 0 and not tf and not sf


def materialize_linears(linears, in_features):
    """Materialises the LazyLinear layers of a chain of layers fed `in_features` inputs, without a forward pass (same default
    init, in the same order, as the reference's first call)."""
    k = in_features
    for m in linears:
        fresh = isinstance(m.weight, torch.nn.parameter.UninitializedParameter)
        if fresh:
            m.in_features = k
            m.weight.materialize((m.out_features, k))
            if m.bias is not None:
                m.bias.materialize((m.out_features,))
            m.reset_parameters()
        elif hasattr(m, "cls_to_become") and m.cls_to_become is not None:
            # a lazy layer whose parameters came from load_state_dict (checkpoint loaded into a fresh model): the
            # tensors exist, but the module still reports in_features = 0 and is still the lazy class
            m.in_features = m.weight.shape[1]
        if fresh or (hasattr(m, "cls_to_become") and m.cls_to_become is not None):
            for hook in ("_initialize_hook", "_load_hook"):  # what LazyModuleMixin._infer_parameters does
                if hasattr(m, hook):
                    getattr(m, hook).remove()
                    delattr(m, hook)
            m.__class__ = m.cls_to_become
        k = m.out_features


def materialized_linears(model):
    """the model's master layers, all of them materialised"""
    lins = model.master_linears()
    if any(isinstance(m.weight, torch.nn.parameter.UninitializedParameter) for m in lins):
        raise RuntimeError("policy has un-materialised LazyLinear layers; call materialize() or run one forward")
    return lins


def upper_bound(model, cache=None):
    """Scalar order upper bound of the policy.  A tensor bound is read back from its device; `cache`, a dict a caller that runs
    every step keeps, holds the value under the tensor's (address, in-place version), so it is read once and not per call."""
    ub = model.warehouse_upper_bound
    if not torch.is_tensor(ub):
        return float(ub)
    if cache is None:
        return float(ub.reshape(-1)[0])
    key = (ub.data_ptr(), ub._version)
    if key not in cache:
        cache.clear()
        cache[key] = float(ub.reshape(-1)[0])
    return cache[key]
