// Stand-alone host program over csrc/horizon_ensemble_plan.h (tests/test_horizon_ensemble_host.py builds it with the host compiler and
// reads its output): one line per query.  <shape> = S Wn Ws Ww ldb T H1 H2 ldw1 ldw2 ldw3 hist_stride (12 numbers), <strides> = the
// 16 NicHorizonEnsemble strides in declaration order.
//   slices <shape>                                                 -> the NicHorizonEnsembleSlices fields in declaration order
//   fwd <shape> head_mode n_models <strides> with_final with_history -> refusal code and reason of the validator
//   bwd <shape> head_mode round_orders n_models <strides>          -> refusal code and reason of the validator
//   offset model stride                                            -> the 64-bit pointer advance of a model
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../neural_inventory_control_amd/csrc/horizon_ensemble_plan.h"

static long long arg(char** v, int i) { return atoll(v[i]); }

static NicHorizonDesc shape(char** v, int i) {
    NicHorizonDesc d;
    memset(&d, 0, sizeof(d));
    NicEnvDims& D = d.io.dims;
    D.n_stores = (int32_t)arg(v, i); D.n_warehouses = (int32_t)arg(v, i + 1);
    D.store_slots = (int32_t)arg(v, i + 2); D.warehouse_slots = (int32_t)arg(v, i + 3);
    D.ldb = (int32_t)arg(v, i + 4);
    d.T = (int32_t)arg(v, i + 5); d.H1 = (int32_t)arg(v, i + 6); d.H2 = (int32_t)arg(v, i + 7);
    d.ldw1 = arg(v, i + 8); d.ldw2 = arg(v, i + 9); d.ldw3 = arg(v, i + 10);
    d.hist_stride = arg(v, i + 11);
    d.n_out = D.n_warehouses ? D.n_warehouses + D.n_stores * D.n_warehouses : D.n_stores;
    return d;
}

static NicHorizonEnsemble strides(char** v, int i) {   // n_models, then the 16 strides
    NicHorizonEnsemble e;
    memset(&e, 0, sizeof(e));
    e.n_models = (int32_t)arg(v, i);
    int64_t* f[16] = {&e.W1, &e.W2, &e.W3, &e.b2, &e.b3, &e.z1_obs, &e.rewards, &e.state_final, &e.state_hist, &e.h1_hist, &e.h2_hist,
                      &e.logits_hist, &e.orders_hist, &e.dz1, &e.dz2, &e.dz3};
    for (int k = 0; k < 16; ++k) *f[k] = arg(v, i + 1 + k);
    return e;
}

static int verdict(int r) {
    printf("%d %s\n", r, nic::horizon_ensemble_reason(r));
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    const char* what = argv[1];
    if (!strcmp(what, "slices") && argc == 14) {
        const NicHorizonEnsembleSlices s = nic::horizon_ensemble_slices(shape(argv, 2));
        const int64_t f[16] = {s.W1, s.W2, s.W3, s.b2, s.b3, s.z1_obs, s.rewards, s.state_final, s.state_hist, s.h1_hist, s.h2_hist,
                               s.logits_hist, s.orders_hist, s.dz1, s.dz2, s.dz3};
        for (int k = 0; k < 16; ++k) printf("%lld%c", (long long)f[k], k == 15 ? '\n' : ' ');
        return 0;
    }
    if (!strcmp(what, "fwd") && argc == 34) {
        NicHorizonDesc d = shape(argv, 2);
        d.head_mode = (int32_t)arg(argv, 14);
        return verdict(nic::horizon_ensemble_check_fwd(d, strides(argv, 15), nic::horizon_ensemble_slices(d), arg(argv, 32) != 0,
                                                       arg(argv, 33) != 0));
    }
    if (!strcmp(what, "bwd") && argc == 33) {
        NicHorizonDesc d = shape(argv, 2);
        d.head_mode = (int32_t)arg(argv, 14);
        d.round_orders = (int32_t)arg(argv, 15);
        return verdict(nic::horizon_ensemble_check_bwd(d, strides(argv, 16), nic::horizon_ensemble_slices(d)));
    }
    if (!strcmp(what, "offset") && argc == 4) {
        printf("%lld\n", (long long)nic::horizon_model_offset((uint32_t)arg(argv, 2), arg(argv, 3)));
        return 0;
    }
    fprintf(stderr, "horizon_ensemble_plan_harness: bad arguments\n");
    return 2;
}
