// Stand-alone program over the active-model mask's host-compilable parts (host compiler alone, no HIP): the request checks of
// csrc/small_ensemble_plan.h (small_ensemble_check_active) and csrc/ensemble_adam_body.h (ea_check_prepare_active /
// ea_check_update_active), the two predicates the kernels branch on, and the recorded kernel name.  Pointers arrive as integers:
// the checks look at addresses only, nothing is dereferenced (the mask's contents live on the device and cannot be checked here).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../neural_inventory_control_amd/csrc/ensemble_adam_body.h"
#include "../neural_inventory_control_amd/csrc/small_ensemble_plan.h"
#include "../neural_inventory_control_amd/csrc/small_rollout_variants.h"

static const void* ptr(const char* s) { return reinterpret_cast<const void*>(static_cast<uintptr_t>(strtoull(s, nullptr, 0))); }
static long long num(const char* s) { return strtoll(s, nullptr, 0); }

int main(int argc, char** argv) {
    using namespace nic;
    if (argc < 2) return 2;
    const char* cmd = argv[1];
    if (!strcmp(cmd, "rollout") && argc == 3) {   // rollout <active>
        const int r = small_ensemble_check_active(ptr(argv[2]));
        printf("%d %s\n", r, small_ensemble_reason(r));
        return 0;
    }
    if (!strcmp(cmd, "prepare") && argc == 12) {   // prepare n_models P hyper max_norm state coef grads grads_stride clip active
        const int r = ea_check_prepare_active((int)num(argv[2]), (int)num(argv[3]), ptr(argv[4]), ptr(argv[5]), ptr(argv[6]), ptr(argv[7]),
                                              ptr(argv[8]), num(argv[9]), ptr(argv[10]), ptr(argv[11]));
        printf("%d %s\n", r, ea_reason(r));
        return 0;
    }
    if (!strcmp(cmd, "update") && argc == 14) {   // update n_models P params stride grads stride exp_avg stride exp_avg_sq stride coef active
        const int r = ea_check_update_active((int)num(argv[2]), (int)num(argv[3]), ptr(argv[4]), num(argv[5]), ptr(argv[6]), num(argv[7]),
                                             ptr(argv[8]), num(argv[9]), ptr(argv[10]), num(argv[11]), ptr(argv[12]), ptr(argv[13]));
        printf("%d %s\n", r, ea_reason(r));
        return 0;
    }
    if (!strcmp(cmd, "runs")) {   // runs <mask entries...>: per model, the kernels' two predicates on the mask, then on NULL
        int32_t mask[64];
        const int n = argc - 2 < 64 ? argc - 2 : 64;
        for (int m = 0; m < n; ++m) mask[m] = (int32_t)num(argv[2 + m]);
        for (int m = 0; m < n; ++m) printf("%d%d ", (int)small_ensemble_model_runs(mask, (uint32_t)m), (int)ea_model_steps(mask, m));
        for (int m = 0; m < n; ++m) printf("%d%d ", (int)small_ensemble_model_runs(nullptr, (uint32_t)m), (int)ea_model_steps(nullptr, m));
        printf("\n");
        return 0;
    }
    if (!strcmp(cmd, "name") && argc == 9) {   // name route width n_hidden shape n_models n_instances active
        char out[160];
        sr_kernel_name(out, sizeof(out), (SrRoute)num(argv[2]), (int)num(argv[3]), (int)num(argv[4]), (int)num(argv[5]), (int)num(argv[6]),
                       (int)num(argv[7]), num(argv[8]) != 0);
        printf("%s\n", out);
        return 0;
    }
    return 2;
}
