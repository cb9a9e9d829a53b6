// Stand-alone host program over the problem-instance part of csrc/small_ensemble_plan.h (tests/test_small_instances_host.py builds
// it with the host compiler and reads its output): one line per query.
//   check n_models n_instances <10 strides> t0 T ldb F <8 table-present flags>  -> refusal code and reason of small_instances_check
//       (strides: demand state0 underage holding lead wh_holding wh_lead wh_edge ech_holding ech_lead, the struct's order)
//   map n_models n_instances                     -> the instance of every model, by the kernels' multiply and shift
//   offsets instance <10 strides>                -> demand and state0 offsets, then the eight tables' as small_instance_tables moves
//                                                   the descriptor's pointers (in floats)
//   magic                                        -> "ok" if the multiply and shift equals m / R for every R in 1..65535 at every
//                                                   model index next to a multiple of R and at 65534, else the first failure
//   name route width n_hidden shape n_models n_instances -> the recorded kernel name
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../neural_inventory_control_amd/csrc/small_ensemble_plan.h"
#include "../neural_inventory_control_amd/csrc/small_rollout_variants.h"

static long long arg(char** v, int i) { return atoll(v[i]); }

static NicSmallInstances instances(int n_instances, char** v, int i) {
    NicSmallInstances in;
    memset(&in, 0, sizeof(in));
    in.n_instances = n_instances;
    in.demand = arg(v, i); in.state0 = arg(v, i + 1);
    in.underage = arg(v, i + 2); in.holding = arg(v, i + 3); in.lead = arg(v, i + 4);
    in.wh_holding = arg(v, i + 5); in.wh_lead = arg(v, i + 6); in.wh_edge = arg(v, i + 7);
    in.ech_holding = arg(v, i + 8); in.ech_lead = arg(v, i + 9);
    return in;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    const char* what = argv[1];
    static float table[8 * 1024];   // (eight regions the descriptor's tables point into: offsets are read back as differences)
    if (!strcmp(what, "check") && argc == 26) {
        const NicSmallInstances in = instances((int)arg(argv, 3), argv, 4);
        NicSmallRolloutDesc d;
        memset(&d, 0, sizeof(d));
        d.t0 = (int32_t)arg(argv, 14); d.T = (int32_t)arg(argv, 15); d.ldb = (int32_t)arg(argv, 16); d.F = (int32_t)arg(argv, 17);
        NicTable2* t[8] = {&d.underage, &d.holding, &d.lead, &d.wh_holding, &d.wh_lead, &d.wh_edge, &d.ech_holding, &d.ech_lead};
        for (int k = 0; k < 8; ++k) t[k]->p = arg(argv, 18 + k) ? table + 1024 * k : nullptr;
        const int r = nic::small_instances_check(in, (int)arg(argv, 2), d);
        printf("%d %s\n", r, nic::small_instances_reason(r));
        return 0;
    }
    if (!strcmp(what, "map") && argc == 4) {
        const int K = (int)arg(argv, 2), R = nic::small_instance_replicas(K, (int)arg(argv, 3));
        const uint64_t magic = nic::small_instance_magic(R);
        for (int m = 0; m < K; ++m) printf("%u%c", nic::small_instance_of((uint32_t)m, magic), m + 1 < K ? ' ' : '\n');
        return 0;
    }
    if (!strcmp(what, "offsets") && argc == 13) {
        const uint32_t instance = (uint32_t)arg(argv, 2);
        const NicSmallInstances in = instances(1, argv, 3);
        NicSmallRolloutDesc d;
        memset(&d, 0, sizeof(d));
        NicTable2* t[8] = {&d.underage, &d.holding, &d.lead, &d.wh_holding, &d.wh_lead, &d.wh_edge, &d.ech_holding, &d.ech_lead};
        for (int k = 0; k < 8; ++k) t[k]->p = table + 1024 * k;
        printf("%lld %lld", (long long)nic::small_instance_offset(instance, in.demand), (long long)nic::small_instance_offset(instance, in.state0));
        nic::small_instance_tables(d, in, instance);
        for (int k = 0; k < 8; ++k) printf(" %lld", (long long)(t[k]->p - (table + 1024 * k)));
        printf("\n");
        return 0;
    }
    if (!strcmp(what, "magic") && argc == 2) {
        for (uint32_t R = 1; R <= 65535; ++R) {
            const uint64_t magic = nic::small_instance_magic((int)R);
            for (uint32_t q = 0; q * R <= 65535; ++q)
                for (int dm = -1; dm <= 1; ++dm) {
                    const int64_t m = (int64_t)q * R + dm;
                    if (m < 0 || m > 65534) continue;
                    if (nic::small_instance_of((uint32_t)m, magic) != (uint32_t)m / R) {
                        printf("m %lld R %u\n", (long long)m, R);
                        return 0;
                    }
                }
            if (nic::small_instance_of(65534u, magic) != 65534u / R) {
                printf("m 65534 R %u\n", R);
                return 0;
            }
        }
        printf("ok\n");
        return 0;
    }
    if (!strcmp(what, "name") && argc == 8) {
        char name[160];
        nic::sr_kernel_name(name, sizeof(name), (nic::SrRoute)arg(argv, 2), (int)arg(argv, 3), (int)arg(argv, 4), (int)arg(argv, 5),
                            (int)arg(argv, 6), (int)arg(argv, 7));
        printf("%s\n", name);
        return 0;
    }
    fprintf(stderr, "small_instances_plan_harness: bad arguments\n");
    return 2;
}
