// Which instantiation of the whole-horizon small-rollout kernels (small_rollout.hip: 32 scenarios per wavefront, small_rollout16.hip:
// 16) runs for a request, and the name that is recorded for it: the ONE place.  Plain C++17 on stack values, for host and device - no
// HIP (tests/small_ensemble_plan_harness.cpp compiles it with the host compiler alone).
#pragma once
#include <stdio.h>
#include <string.h>

#include <type_traits>

#include "../../include/nic_rollout.h"

namespace nic {

// Chain shapes: the two chains the reference ships are compiled with their structure as constants (see sr_fix_shape in
// small_rollout_mfma.h for why), every other supported chain runs the run-time-structure kernels.
//   SR_ANY:       any supported chain
//   SR_ONE_STORE: one store, Ws = 4, softplus head                          (one_store_lost.yml / one_store_backlogged.yml + vanilla_one_store)
//   SR_SERIAL:    store + warehouse + 2 echelons, 4 / 3 / 4, serial head    (serial_system.yml + vanilla_serial)
enum SrShape { SR_ANY = 0, SR_ONE_STORE = 1, SR_SERIAL = 2 };
inline int sr_shape_of(const NicSmallRolloutDesc& d) {
    if (d.Ws == 4 && d.Wn == 0 && d.E == 0 && d.head == 0 && d.F == 4 && d.n_out == 1) return SR_ONE_STORE;
    if (d.Ws == 4 && d.Wn == 1 && d.Ww == 3 && d.E == 2 && d.We == 4 && d.head == 1 && d.F == 15 && d.n_out == 4) return SR_SERIAL;
    return SR_ANY;
}
inline const char* sr_shape_name(int shape) { return shape == SR_ONE_STORE ? "one_store" : (shape == SR_SERIAL ? "serial" : "any"); }

// scenarios per wavefront: 32 unless the descriptor asks for the 16-scenario form (whose history is in a wave-native order private
// to its forward / backward pair, so the choice is the caller's and the same for both launches)
inline int sr_lane_width(const NicSmallRolloutDesc& d) { return d.lane_scenarios == 16 ? 16 : 32; }

// The three routes.  SR_BWD_DZ, the backward sweep that writes a dz history for per-layer weight-gradient GEMMs, is the referee of
// the in-kernel weight gradients: 32 scenarios per wavefront and one model only.
enum SrRoute { SR_FWD = 0, SR_BWD_WGRAD = 1, SR_BWD_DZ = 2 };

// (route, chain shape, n_hidden) -> the instantiation <NL, SHAPE>.  The structure is compiled in for both shipped chains at two and
// three hidden layers; everything else is the run-time-structure kernel of that depth.
// DECISION: the dz-history route compiles in only the depths the shipped policies have - (one_store, 3) and (serial, 2).  Its
// (one_store, 2) and (serial, 3) requests run the run-time-structure kernel: five instantiations of a referee-only route, not seven.
struct SrVariant { int nl, shape; };
constexpr SrVariant sr_variant(SrRoute route, int shape, int n_hidden) {
    const bool compiled_in = route == SR_BWD_DZ ? (shape == SR_ONE_STORE && n_hidden == 3) || (shape == SR_SERIAL && n_hidden == 2)
                                                : (shape == SR_ONE_STORE || shape == SR_SERIAL) && (n_hidden == 2 || n_hidden == 3);
    return SrVariant{n_hidden, compiled_in ? shape : SR_ANY};
}

// The recorded kernel name (nic_last_kernel()).  It states the REQUEST - width, n_hidden, the chain's shape class, the models of an
// ensemble launch (n_models 0: the single-model entry points), the instances of a launch through nic_small_rollout_instances_*
// (n_instances 0: every other entry point), `active` for a launch through the *_active entry points -, so the two dz-history cells without a kernel of their own are recorded under their
// shape's name.
inline void sr_kernel_name(char* out, size_t size, SrRoute route, int width, int n_hidden, int shape, int n_models, int n_instances = 0,
                           bool active = false) {
    const char* kernel = route == SR_FWD ? (width == 16 ? "small_rollout16_fwd_kernel" : "small_rollout_fwd_mfma_kernel")
                                         : (width == 16 ? "small_rollout16_bwd_kernel" : "small_rollout_bwd_mfma_kernel");
    const char* wgrad = route == SR_BWD_WGRAD ? "wgrad," : "";
    if (n_models > 0 && n_instances > 0)
        snprintf(out, size, "%s<%d,%s%s,models=%d,instances=%d>", kernel, n_hidden, wgrad, sr_shape_name(shape), n_models, n_instances);
    else if (n_models > 0) snprintf(out, size, "%s<%d,%s%s,models=%d>", kernel, n_hidden, wgrad, sr_shape_name(shape), n_models);
    else snprintf(out, size, "%s<%d,%s%s>", kernel, n_hidden, wgrad, sr_shape_name(shape));
    if (active) {
        const size_t n = strlen(out);
        if (n >= 1 && n + 8 <= size) snprintf(out + n - 1, size - n + 1, ",active>");
    }
}

// Run-time variant -> compile-time constants: calls f(integral_constant<int, NL>, integral_constant<int, SHAPE>, bool_constant<ENS>)
// for the cell that matches and returns true; false if the route has no such instantiation (the dz-history route has no ensemble
// form).  f is a generic callable that launches kernel<NL, SHAPE, ENS>; it is instantiated for exactly the cells sr_variant can
// return for ROUTE (x one model / K models where the route has both), so the set of kernels in a code object follows from
// sr_variant and from nothing else (the launchers add, for every ENS cell, its twin that tests the active-model mask).  (The cells are tried in the order the kernels have always had in the code objects.)
template <SrRoute ROUTE, int NL, int SHAPE, class F>
inline bool sr_dispatch_cell(SrVariant v, bool ensemble, F& f) {
    if constexpr (sr_variant(ROUTE, SHAPE, NL).shape == SHAPE) {
        if (v.nl != NL || v.shape != SHAPE) return false;
        using nl = std::integral_constant<int, NL>;
        using sh = std::integral_constant<int, SHAPE>;
        if constexpr (ROUTE == SR_BWD_DZ) {
            if (ensemble) return false;
        } else if (ensemble) {
            f(nl{}, sh{}, std::true_type{});
            return true;
        }
        f(nl{}, sh{}, std::false_type{});
        return true;
    } else {
        return false;
    }
}
template <SrRoute ROUTE, class F>
inline bool sr_dispatch(SrVariant v, bool ensemble, F f) {
    return sr_dispatch_cell<ROUTE, 3, SR_ONE_STORE>(v, ensemble, f) || sr_dispatch_cell<ROUTE, 2, SR_ONE_STORE>(v, ensemble, f) ||
           sr_dispatch_cell<ROUTE, 2, SR_SERIAL>(v, ensemble, f) || sr_dispatch_cell<ROUTE, 3, SR_SERIAL>(v, ensemble, f) ||
           sr_dispatch_cell<ROUTE, 1, SR_ANY>(v, ensemble, f) || sr_dispatch_cell<ROUTE, 2, SR_ANY>(v, ensemble, f) ||
           sr_dispatch_cell<ROUTE, 3, SR_ANY>(v, ensemble, f);
}

}  // namespace nic
