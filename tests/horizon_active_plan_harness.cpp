// Stand-alone host program over the active-model mask's side of csrc/horizon_ensemble_plan.h and csrc/linear_models_plan.h
// (tests/test_horizon_active_host.py builds it with the host compiler and reads its output): one line per answer, fields separated
// by '|'.  Addresses are plain integers (only null-ness and the low bits count).
//   he_active ADDR              -> code|reason of horizon_ensemble_check_active
//   he_runs                     -> horizon_ensemble_model_runs / linear_model_runs over the host mask {1, 0, 7} and over NULL, models 0..2
//   he_reasons                  -> code|reason for HE_OK .. HE_ACTIVE, one per line
//   lm_fwd ACTIVE [Y_STRIDE]    -> code|reason of linear_models_check_fwd for a good request of 3 models (Y_STRIDE: a bad one instead)
//   lm_wgrad ACTIVE [X_STRIDE]  -> the same for linear_models_check_wgrad
//   lm_reduce ACTIVE [N_SPLITS] -> the same for linear_models_check_reduce
//   lm_plans ACTIVE             -> the refusal of linear_models_fwd_plan | of linear_models_wgrad_plan for the same requests (256 CUs)
//   lm_reasons                  -> code|reason for LM_OK .. LM_MASK, one per line, then "end|" LM_REFUSAL_END "|" LM_ACTIVE_REFUSAL_END
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../neural_inventory_control_amd/csrc/horizon_ensemble_plan.h"
#include "../neural_inventory_control_amd/csrc/linear_models_plan.h"

static long long arg(char** v, int i) { return atoll(v[i]); }

// 3 models of a 17 x 41 layer over 140 columns, as tests/test_gpu_linear_models.py's refusal test lays them out
static const int M = 3, N = 17, K = 41, COLS = 140, LDW = 44, LDS = 44, SPLITS = 3;
static nic::LmFwdRequest fwd_request(uint64_t active) {
    return nic::LmFwdRequest{1024, 2048, 4096, 8192, LDW, N * LDW + 8, N + 3, K * COLS + 8, N * COLS + 8, N, K, COLS, COLS, NIC_ACT_ELU, M, active};
}
static nic::LmWgradRequest wgrad_request(uint64_t active) {
    return nic::LmWgradRequest{1024, 4096, 8192, N * COLS + 8, K * COLS + 8, SPLITS * N * LDS + 8, LDS, N, K, COLS, COLS, SPLITS, M, active};
}
static nic::LmReduceRequest reduce_request(uint64_t active) {
    return nic::LmReduceRequest{8192, 1024, 2048, SPLITS * N * LDS + 8, LDS, K, N * K + 5, N + 3, N, K, SPLITS, M, active};
}
static int say(int code) {
    printf("%d|%s\n", code, nic::linear_models_reason(code));
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    const char* what = argv[1];
    if (!strcmp(what, "he_active") && argc == 3) {
        const int code = nic::horizon_ensemble_check_active(reinterpret_cast<const void*>((uintptr_t)arg(argv, 2)));
        printf("%d|%s\n", code, nic::horizon_ensemble_reason(code));
        return 0;
    }
    if (!strcmp(what, "he_runs") && argc == 2) {
        const int32_t mask[3] = {1, 0, 7};
        for (uint32_t m = 0; m < 3; ++m)
            printf("%d %d %d %d\n", (int)nic::horizon_ensemble_model_runs(mask, m), (int)nic::horizon_ensemble_model_runs(nullptr, m),
                   (int)nic::linear_model_runs(mask, m), (int)nic::linear_model_runs(nullptr, m));
        return 0;
    }
    if (!strcmp(what, "he_reasons") && argc == 2) {
        for (int c = 0; c <= nic::HE_ACTIVE; ++c) printf("%d|%s\n", c, nic::horizon_ensemble_reason(c));
        return 0;
    }
    if (!strcmp(what, "lm_fwd") && (argc == 3 || argc == 4)) {
        nic::LmFwdRequest r = fwd_request((uint64_t)arg(argv, 2));
        if (argc == 4) r.Y_stride = arg(argv, 3);
        return say(nic::linear_models_check_fwd(r));
    }
    if (!strcmp(what, "lm_wgrad") && (argc == 3 || argc == 4)) {
        nic::LmWgradRequest r = wgrad_request((uint64_t)arg(argv, 2));
        if (argc == 4) r.X_stride = arg(argv, 3);
        return say(nic::linear_models_check_wgrad(r));
    }
    if (!strcmp(what, "lm_reduce") && (argc == 3 || argc == 4)) {
        nic::LmReduceRequest r = reduce_request((uint64_t)arg(argv, 2));
        if (argc == 4) r.n_splits = (int)arg(argv, 3);
        return say(nic::linear_models_check_reduce(r));
    }
    if (!strcmp(what, "lm_plans") && argc == 3) {
        printf("%d|%d\n", nic::linear_models_fwd_plan(fwd_request((uint64_t)arg(argv, 2)), 256).refusal,
               nic::linear_models_wgrad_plan(wgrad_request((uint64_t)arg(argv, 2))).refusal);
        return 0;
    }
    if (!strcmp(what, "lm_reasons") && argc == 2) {
        for (int c = 0; c <= nic::LM_MASK; ++c) printf("%d|%s\n", c, nic::linear_models_reason(c));
        printf("end|%d|%d\n", (int)nic::LM_REFUSAL_END, (int)nic::LM_ACTIVE_REFUSAL_END);
        return 0;
    }
    fprintf(stderr, "horizon_active_plan_harness: bad arguments\n");
    return 2;
}
