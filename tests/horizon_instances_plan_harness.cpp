// Stand-alone host program over the problem-instance part of csrc/horizon_ensemble_plan.h (tests/test_horizon_instances_host.py builds
// it with the host compiler and reads its output): one line per query.  <shape> = S Wn Ws Ww B ldb T t0 (8 numbers), <strides> = the
// 8 NicHorizonInstances strides in declaration order (demand state0 underage holding lead wh_holding wh_lead wh_edge), <tables> = per
// table of that order "present loc_stride scn_stride" (lead: "present loc_stride sup_stride scn_stride"): 19 numbers.
//   check n_models n_instances <strides> <shape> <tables> -> refusal code and reason of horizon_instances_check
//   slices <shape> <tables>                       -> the demand and state0 slices, then the six tables' extents
//   map n_models n_instances                      -> the instance of every model: the rule (m / R) and the kernels' multiply and shift
//   offsets instance <strides>                    -> demand and state0 offsets, then the six tables' as horizon_instance_tables moves
//                                                    the descriptor's pointers (in floats); a NULL table with stride 0 stays NULL
//   magic                                         -> "ok" if the multiply and shift equals m / R for every R in 1..65535 at every
//                                                    model index next to a multiple of R and at 65534, else the first failure
//   shared <strides>                              -> 1 if NicHorizonInstances{1, strides} equals horizon_instances_shared() byte for byte
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../neural_inventory_control_amd/csrc/horizon_ensemble_plan.h"

static long long arg(char** v, int i) { return atoll(v[i]); }
static float table[6 * 4096];   // (six regions the descriptor's tables point into: offsets are read back as differences)

static NicHorizonInstances instances(int n_instances, char** v, int i) {
    NicHorizonInstances in;
    memset(&in, 0, sizeof(in));
    in.n_instances = n_instances;
    in.demand = arg(v, i); in.state0 = arg(v, i + 1);
    in.underage = arg(v, i + 2); in.holding = arg(v, i + 3); in.lead = arg(v, i + 4);
    in.wh_holding = arg(v, i + 5); in.wh_lead = arg(v, i + 6); in.wh_edge = arg(v, i + 7);
    return in;
}

static NicHorizonDesc shape(char** v, int i) {   // 8 shape numbers, then the 19 of the tables
    NicHorizonDesc d;
    memset(&d, 0, sizeof(d));
    NicEnvDims& D = d.io.dims;
    D.n_stores = (int32_t)arg(v, i); D.n_warehouses = (int32_t)arg(v, i + 1);
    D.store_slots = (int32_t)arg(v, i + 2); D.warehouse_slots = (int32_t)arg(v, i + 3);
    D.n_scenarios = (int32_t)arg(v, i + 4); D.ldb = (int32_t)arg(v, i + 5);
    d.T = (int32_t)arg(v, i + 6); d.t0 = (int32_t)arg(v, i + 7);
    i += 8;
    NicTable2* t2[6] = {&d.io.underage, &d.io.holding, nullptr, &d.io.wh_holding, &d.io.wh_lead_times, &d.io.wh_edge_costs};
    for (int k = 0; k < 6; ++k) {
        const float* p = arg(v, i) ? table + 4096 * k : nullptr;
        if (k == 2) {
            d.io.lead_times.p = p;
            d.io.lead_times.loc_stride = arg(v, i + 1); d.io.lead_times.sup_stride = arg(v, i + 2); d.io.lead_times.scn_stride = arg(v, i + 3);
            i += 4;
        } else {
            t2[k]->p = p;
            t2[k]->loc_stride = arg(v, i + 1); t2[k]->scn_stride = arg(v, i + 2);
            i += 3;
        }
    }
    return d;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    const char* what = argv[1];
    if (!strcmp(what, "check") && argc == 4 + 8 + 8 + 19) {
        const NicHorizonInstances in = instances((int)arg(argv, 3), argv, 4);
        const NicHorizonDesc d = shape(argv, 12);
        const int r = nic::horizon_instances_check(in, (int)arg(argv, 2), d);
        printf("%d %s\n", r, nic::horizon_instances_reason(r));
        return 0;
    }
    if (!strcmp(what, "slices") && argc == 2 + 8 + 19) {
        const NicHorizonDesc d = shape(argv, 2);
        printf("%lld %lld", (long long)nic::horizon_instance_demand_slice(d), (long long)nic::horizon_instance_state0_slice(d));
        for (int k = 0; k < nic::kHiTables; ++k) printf(" %lld", (long long)nic::horizon_instance_table_extent(d, k));
        printf("\n");
        return 0;
    }
    if (!strcmp(what, "map") && argc == 4) {
        const int K = (int)arg(argv, 2), R = nic::horizon_instance_replicas(K, (int)arg(argv, 3));
        const uint64_t magic = nic::horizon_instance_magic(R);
        for (int m = 0; m < K; ++m) {
            const uint32_t rule = nic::horizon_instance_of((uint32_t)m, (uint32_t)R);
            if (rule != nic::horizon_instance_by_magic((uint32_t)m, magic)) {
                printf("mismatch at model %d\n", m);
                return 0;
            }
            printf("%u%c", rule, m + 1 < K ? ' ' : '\n');
        }
        return 0;
    }
    if (!strcmp(what, "offsets") && argc == 11) {
        const uint32_t instance = (uint32_t)arg(argv, 2);
        const NicHorizonInstances in = instances(1, argv, 3);
        NicEnvStepIO io;
        memset(&io, 0, sizeof(io));
        const float** p[6] = {&io.underage.p, &io.holding.p, &io.lead_times.p, &io.wh_holding.p, &io.wh_lead_times.p, &io.wh_edge_costs.p};
        // (a table whose stride is 0 is left NULL here: what the validator guarantees of a NULL table)
        for (int k = 0; k < 6; ++k) *p[k] = nic::horizon_instance_table_stride(in, k) ? table + 4096 * k : nullptr;
        printf("%lld %lld", (long long)nic::horizon_instance_offset(instance, in.demand), (long long)nic::horizon_instance_offset(instance, in.state0));
        nic::horizon_instance_tables(io, in, instance);
        for (int k = 0; k < 6; ++k) {
            if (nic::horizon_instance_table_stride(in, k)) printf(" %lld", (long long)(*p[k] - (table + 4096 * k)));
            else printf(" %s", *p[k] == nullptr ? "null" : "moved");
        }
        printf("\n");
        return 0;
    }
    if (!strcmp(what, "magic") && argc == 2) {
        for (uint32_t R = 1; R <= 65535; ++R) {
            const uint64_t magic = nic::horizon_instance_magic((int)R);
            for (uint32_t q = 0; q * R <= 65535; ++q)
                for (int dm = -1; dm <= 1; ++dm) {
                    const int64_t m = (int64_t)q * R + dm;
                    if (m < 0 || m > 65534) continue;
                    if (nic::horizon_instance_by_magic((uint32_t)m, magic) != nic::horizon_instance_of((uint32_t)m, R)) {
                        printf("m %lld R %u\n", (long long)m, R);
                        return 0;
                    }
                }
            if (nic::horizon_instance_by_magic(65534u, magic) != 65534u / R) {
                printf("m 65534 R %u\n", R);
                return 0;
            }
        }
        printf("ok\n");
        return 0;
    }
    if (!strcmp(what, "shared") && argc == 10) {
        const NicHorizonInstances in = instances(1, argv, 2), want = nic::horizon_instances_shared();
        printf("%d\n", memcmp(&in, &want, sizeof(in)) == 0 ? 1 : 0);
        return 0;
    }
    fprintf(stderr, "horizon_instances_plan_harness: bad arguments\n");
    return 2;
}
