// Stand-alone host program over csrc/linear_models_plan.h (tests/test_linear_models_host.py builds it with the host compiler and reads
// its output): one line per query, fields separated by '|'.  Addresses are plain integers (only null-ness and the low 4 bits count).
//   fwd W bias X Y ldw W_stride bias_stride X_stride Y_stride N K n_scenarios ldb act n_models cus
//       -> code|reason|operands kernel grid|operands kernel grid   (the model plan, then nic_linear_fwd's plan for model 0's operands)
//   wgrad dY X slab dY_stride X_stride slab_stride lds N K n_scenarios ldb n_splits n_models
//       -> code|reason|buffer dma tile slots chunk|buffer dma tile slots chunk   (the model plan, then nic_linear_wgrad's)
//   reduce slab dW db slab_stride lds lddw dW_stride db_stride N K n_splits n_models -> code|reason|wide
//   offset model stride                                            -> the 64-bit pointer advance of a model
//   reasons                                                        -> code|reason for every refusal code, one per line
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../neural_inventory_control_amd/csrc/linear_models_plan.h"

static long long arg(char** v, int i) { return atoll(v[i]); }

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    const char* what = argv[1];
    if (!strcmp(what, "fwd") && argc == 18) {
        const nic::LmFwdRequest r{(uint64_t)arg(argv, 2), (uint64_t)arg(argv, 3), (uint64_t)arg(argv, 4), (uint64_t)arg(argv, 5),
                                  arg(argv, 6), arg(argv, 7), arg(argv, 8), arg(argv, 9), arg(argv, 10), (int)arg(argv, 11),
                                  (int)arg(argv, 12), (int)arg(argv, 13), (int)arg(argv, 14), (int)arg(argv, 15), (int)arg(argv, 16)};
        const int cus = (int)arg(argv, 17);
        const nic::LmFwdPlan p = nic::linear_models_fwd_plan(r, cus);
        printf("%d|%s", p.refusal, nic::linear_models_reason(p.refusal));
        if (p.refusal == nic::LM_OK || p.refusal == nic::LM_PLAN) {
            // what nic_linear_fwd computes for model 0's operands
            const bool operands = nic::wx_operands(r.W | r.X, r.ldw, r.ldb, r.N, r.K);
            const nic::WxPlan one = nic::wx_plan(r.N, r.K, (r.n_scenarios + 3) / 4 * 4, operands, cus);
            printf("|%d %d %d|%d %d %d", (int)p.operands, (int)p.plan.kernel, p.plan.grid, (int)operands, (int)one.kernel, one.grid);
        }
        printf("\n");
        return 0;
    }
    if (!strcmp(what, "wgrad") && argc == 15) {
        const nic::LmWgradRequest r{(uint64_t)arg(argv, 2), (uint64_t)arg(argv, 3), (uint64_t)arg(argv, 4), arg(argv, 5), arg(argv, 6),
                                    arg(argv, 7), arg(argv, 8), (int)arg(argv, 9), (int)arg(argv, 10), (int)arg(argv, 11),
                                    (int)arg(argv, 12), (int)arg(argv, 13), (int)arg(argv, 14)};
        const nic::LmWgradPlan p = nic::linear_models_wgrad_plan(r);
        printf("%d|%s", p.refusal, nic::linear_models_reason(p.refusal));
        if (p.refusal == nic::LM_OK || p.refusal == nic::LM_PLAN) {
            // what nic_linear_wgrad computes for model 0's operands
            const nic::WgradOperands ops = nic::wgrad_operands(r.dY | r.X, r.slab, r.ldb, r.lds, r.N, r.K);
            const nic::WgradPlan one = nic::wgrad_plan(nic::WG_ONE_PERIOD, r.N, r.K, r.n_scenarios, 1, r.n_splits, ops);
            printf("|%d %d %d %d %d|%d %d %d %d %d", (int)p.operands.buffer, (int)p.operands.dma, (int)nic::wgrad_launch(p.plan, 1, 0).tile,
                   p.plan.slots, p.plan.chunk, (int)ops.buffer, (int)ops.dma, (int)nic::wgrad_launch(one, 1, 0).tile, one.slots, one.chunk);
        }
        printf("\n");
        return 0;
    }
    if (!strcmp(what, "reduce") && argc == 14) {
        const nic::LmReduceRequest r{(uint64_t)arg(argv, 2), (uint64_t)arg(argv, 3), (uint64_t)arg(argv, 4), arg(argv, 5), arg(argv, 6),
                                     arg(argv, 7), arg(argv, 8), arg(argv, 9), (int)arg(argv, 10), (int)arg(argv, 11), (int)arg(argv, 12),
                                     (int)arg(argv, 13)};
        const int code = nic::linear_models_check_reduce(r);
        printf("%d|%s|%d\n", code, nic::linear_models_reason(code), (int)nic::wgrad_reduce_wide(r.n_splits, r.N, r.K));
        return 0;
    }
    if (!strcmp(what, "offset") && argc == 4) {
        printf("%lld\n", (long long)nic::linear_model_offset((uint32_t)arg(argv, 2), arg(argv, 3)));
        return 0;
    }
    if (!strcmp(what, "reasons") && argc == 2) {
        for (int c = 0; c < nic::LM_REFUSAL_END; ++c) printf("%d|%s\n", c, nic::linear_models_reason(c));
        return 0;
    }
    fprintf(stderr, "linear_models_plan_harness: bad arguments\n");
    return 2;
}
