// Stand-alone host program over csrc/small_ensemble_plan.h (tests/test_small_ensemble_host.py builds it with the host compiler and
// reads its output): one line per query.
//   slices B ldb T F n_hidden n_out width        -> the NicSmallEnsembleSlices fields in declaration order
//   scratch n_rows P n_reward_elems              -> floats of the reduction's scratch
//   fwd / bwd / reduce ...                       -> refusal code and reason of the validator
// and over csrc/small_rollout_variants.h (route: 0 forward, 1 backward with weight gradients, 2 dz-history backward; shape: 0 any, 1
// one_store, 2 serial):
//   classify Ws Wn Ww E We head F n_out lanes    -> shape name and scenarios per wavefront of a descriptor
//   variant route shape n_hidden                 -> NL and shape name of the instantiation
//   name route width n_hidden shape n_models     -> the recorded kernel name (n_models 0: a single-model entry point)
//   dispatch route shape n_hidden ensemble       -> the constants the dispatcher hands its callable ("NL SHAPE ENS"), or "none"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../neural_inventory_control_amd/csrc/small_ensemble_plan.h"
#include "../neural_inventory_control_amd/csrc/small_rollout_variants.h"

static long long arg(char** v, int i) { return atoll(v[i]); }

static NicSmallEnsemble strides(char** v, int i) {   // n_models weights rewards final states hidden logits slab grad scratch
    NicSmallEnsemble e;
    memset(&e, 0, sizeof(e));
    e.n_models = (int32_t)arg(v, i);
    e.weights = arg(v, i + 1); e.rewards = arg(v, i + 2); e.final_state = arg(v, i + 3);
    e.states = arg(v, i + 4); e.hidden = arg(v, i + 5); e.logits = arg(v, i + 6);
    e.slab = arg(v, i + 7); e.grad = arg(v, i + 8); e.scratch = arg(v, i + 9);
    return e;
}

static NicSmallEnsembleSlices slices(char** v, int i) {
    return nic::small_ensemble_slices((int)arg(v, i), (int)arg(v, i + 1), (int)arg(v, i + 2), (int)arg(v, i + 3), (int)arg(v, i + 4),
                                      (int)arg(v, i + 5), (int)arg(v, i + 6));
}

static int verdict(int r) {
    printf("%d %s\n", r, nic::small_ensemble_reason(r));
    return 0;
}

template <nic::SrRoute ROUTE>
static int dispatch(int shape, int n_hidden, bool ensemble) {
    const bool found = nic::sr_dispatch<ROUTE>(nic::sr_variant(ROUTE, shape, n_hidden), ensemble, [](auto nl, auto sh, auto ens) {
        printf("%d %d %d\n", (int)nl(), (int)sh(), (int)ens());
    });
    if (!found) printf("none\n");
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    const char* what = argv[1];
    if (!strcmp(what, "slices") && argc == 9) {
        const NicSmallEnsembleSlices s = slices(argv, 2);
        printf("%lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld\n", (long long)s.weights, (long long)s.rewards,
               (long long)s.final_state, (long long)s.states, (long long)s.hidden, (long long)s.logits, (long long)s.slab_rows,
               (long long)s.slab_row_stride, (long long)s.slab, (long long)s.grad, (long long)s.scratch);
        return 0;
    }
    if (!strcmp(what, "scratch") && argc == 5) {
        printf("%d\n", nic::sr_reduce_scratch((int)arg(argv, 2), (int)arg(argv, 3), arg(argv, 4)));
        return 0;
    }
    // fwd <7 shape numbers> <10 strides> with_history
    if (!strcmp(what, "fwd") && argc == 20) return verdict(nic::small_ensemble_check_fwd(strides(argv, 9), slices(argv, 2), arg(argv, 19) != 0));
    // bwd <7 shape numbers> <10 strides> slab_row_stride
    if (!strcmp(what, "bwd") && argc == 20) return verdict(nic::small_ensemble_check_bwd(strides(argv, 9), slices(argv, 2), arg(argv, 19)));
    // reduce <10 strides> with_slab n_rows slab_row_stride P with_rewards n_reward_elems
    if (!strcmp(what, "reduce") && argc == 18)
        return verdict(nic::small_ensemble_check_reduce(strides(argv, 2), arg(argv, 12) != 0, (int)arg(argv, 13), arg(argv, 14), (int)arg(argv, 15),
                                                        arg(argv, 16) != 0, arg(argv, 17)));
    if (!strcmp(what, "classify") && argc == 11) {
        NicSmallRolloutDesc d;
        memset(&d, 0, sizeof(d));
        d.Ws = (int32_t)arg(argv, 2); d.Wn = (int32_t)arg(argv, 3); d.Ww = (int32_t)arg(argv, 4); d.E = (int32_t)arg(argv, 5);
        d.We = (int32_t)arg(argv, 6); d.head = (int32_t)arg(argv, 7); d.F = (int32_t)arg(argv, 8); d.n_out = (int32_t)arg(argv, 9);
        d.lane_scenarios = (int32_t)arg(argv, 10);
        printf("%s %d\n", nic::sr_shape_name(nic::sr_shape_of(d)), nic::sr_lane_width(d));
        return 0;
    }
    if (!strcmp(what, "variant") && argc == 5) {
        const nic::SrVariant v = nic::sr_variant((nic::SrRoute)arg(argv, 2), (int)arg(argv, 3), (int)arg(argv, 4));
        printf("%d %s\n", v.nl, nic::sr_shape_name(v.shape));
        return 0;
    }
    if (!strcmp(what, "name") && argc == 7) {
        char name[160];
        nic::sr_kernel_name(name, sizeof(name), (nic::SrRoute)arg(argv, 2), (int)arg(argv, 3), (int)arg(argv, 4), (int)arg(argv, 5),
                            (int)arg(argv, 6));
        printf("%s\n", name);
        return 0;
    }
    if (!strcmp(what, "dispatch") && argc == 6) {
        const int shape = (int)arg(argv, 3), n_hidden = (int)arg(argv, 4);
        const bool ensemble = arg(argv, 5) != 0;
        switch (arg(argv, 2)) {
            case nic::SR_FWD: return dispatch<nic::SR_FWD>(shape, n_hidden, ensemble);
            case nic::SR_BWD_WGRAD: return dispatch<nic::SR_BWD_WGRAD>(shape, n_hidden, ensemble);
            case nic::SR_BWD_DZ: return dispatch<nic::SR_BWD_DZ>(shape, n_hidden, ensemble);
        }
    }
    fprintf(stderr, "small_ensemble_plan_harness: bad arguments\n");
    return 2;
}
