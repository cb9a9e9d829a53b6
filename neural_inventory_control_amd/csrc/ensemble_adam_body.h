// Adam for K models whose parameters are the rows of one [K][P] buffer (nic_ensemble_adam_*, csrc/ensemble_adam.hip): the per-model
// preparation of a step, the per-element update and the checks a request has to pass before anything is launched - each written
// ONCE, here.  Plain C++ on values the caller hands in, for host and device - no HIP, no allocation
// (tests/ensemble_adam_harness.cpp compiles it with the host compiler alone and is the referee of the kernels, bit for bit).
//
// One step is two passes in stream order.  `ea_prepare` (per model, all in double) advances the step counter and the running
// products c1 = beta1^t, c2 = beta2^t and rounds the step's coefficients to float once; `ea_update` (per element, all in float)
// reads those coefficients only, so the counter is never read while it advances.  The products are running: there is no `pow`,
// on which the host and device maths libraries differ, while double *, / and sqrt are IEEE on both.
#pragma once
#include <math.h>
#include <stdint.h>
#include "../../include/nic_rollout.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define NIC_EA_FN __host__ __device__ inline
#else
#define NIC_EA_FN inline
#endif

namespace nic {

constexpr int kEaMaxModels = 65535;   // grid y of the update
constexpr int kEaThreads = 256;       // threads per workgroup: models per workgroup (prepare), columns per workgroup (update)

// one model's row of the hyper-parameter table (doubles)
enum EaHyper { EA_LR = 0, EA_BETA1, EA_BETA2, EA_EPS, EA_WEIGHT_DECAY, EA_HYPER_COUNT };
using EaState = NicEnsembleAdamState;   // one model's state: the step counter and the running products beta1^step, beta2^step
// one model's row of the coefficient table (floats), what the update reads
enum EaCoef { EA_STEP_SIZE = 0, EA_INV_BC2_SQRT, EA_B1, EA_ONE_MINUS_B1, EA_B2, EA_ONE_MINUS_B2, EA_EPSILON, EA_DECAY, EA_COEF_COUNT };

// ---- per model: the next step's coefficients -------------------------------------------------------------------------------------
NIC_EA_FN void ea_prepare(const double* hyper, EaState* state, float* coef) {
    const double lr = hyper[EA_LR], beta1 = hyper[EA_BETA1], beta2 = hyper[EA_BETA2];
    const double c1 = state->c1 * beta1, c2 = state->c2 * beta2;
    state->step += 1;
    state->c1 = c1;
    state->c2 = c2;
    coef[EA_STEP_SIZE] = (float)(lr / (1.0 - c1));
    coef[EA_INV_BC2_SQRT] = (float)(1.0 / sqrt(1.0 - c2));
    coef[EA_B1] = (float)beta1;
    coef[EA_ONE_MINUS_B1] = (float)(1.0 - beta1);
    coef[EA_B2] = (float)beta2;
    coef[EA_ONE_MINUS_B2] = (float)(1.0 - beta2);
    coef[EA_EPSILON] = (float)hyper[EA_EPS];
    coef[EA_DECAY] = (float)hyper[EA_WEIGHT_DECAY];
}

// ---- per element: the update (float32; the units that include this are built with -ffp-contract=off) ----------------------------
NIC_EA_FN void ea_update(float* p, float g, float* exp_avg, float* exp_avg_sq, const float* coef) {
    const float decay = coef[EA_DECAY];
    const float gd = decay != 0.f ? g + decay * *p : g;
    const float m = coef[EA_B1] * *exp_avg + coef[EA_ONE_MINUS_B1] * gd;
    const float v = coef[EA_B2] * *exp_avg_sq + coef[EA_ONE_MINUS_B2] * (gd * gd);
    *exp_avg = m;
    *exp_avg_sq = v;
    *p -= coef[EA_STEP_SIZE] * (m / (sqrtf(v) * coef[EA_INV_BC2_SQRT] + coef[EA_EPSILON]));
}

// ---- checks ----------------------------------------------------------------------------------------------------------------------
// what a request is refused for (0: accepted); ea_reason names them
enum EaRefusal { EA_OK = 0, EA_MODELS, EA_COLUMNS, EA_NULL, EA_PARAMS_STRIDE, EA_GRADS_STRIDE, EA_EXP_AVG_STRIDE, EA_EXP_AVG_SQ_STRIDE,
                 EA_ACTIVE, EA_CLIP_TOGETHER };
NIC_EA_FN const char* ea_reason(int r) {
    switch (r) {
        case EA_OK: return "accepted";
        case EA_MODELS: return "n_models must be 1..65535";
        case EA_COLUMNS: return "P must be at least 1";
        case EA_NULL: return "null pointer";
        case EA_PARAMS_STRIDE: return "parameter stride shorter than P";
        case EA_GRADS_STRIDE: return "gradient stride shorter than P";
        case EA_EXP_AVG_STRIDE: return "exp_avg stride shorter than P";
        case EA_EXP_AVG_SQ_STRIDE: return "exp_avg_sq stride shorter than P";
        case EA_ACTIVE: return "the active mask must be NULL or 4-byte aligned";
        case EA_CLIP_TOGETHER: return "max_norm, clip and the gradients go together";
        default: return "?";
    }
}
NIC_EA_FN int ea_check_prepare(int n_models, const void* hyper, const void* state, const void* coef) {
    if (n_models < 1 || n_models > kEaMaxModels) return EA_MODELS;
    if (!hyper || !state || !coef) return EA_NULL;
    return EA_OK;
}
NIC_EA_FN int ea_check_update(int n_models, int P, const void* params, int64_t params_stride, const void* grads, int64_t grads_stride,
                              const void* exp_avg, int64_t exp_avg_stride, const void* exp_avg_sq, int64_t exp_avg_sq_stride,
                              const void* coef) {
    if (n_models < 1 || n_models > kEaMaxModels) return EA_MODELS;
    if (P < 1) return EA_COLUMNS;
    if (!params || !grads || !exp_avg || !exp_avg_sq || !coef) return EA_NULL;
    if (params_stride < P) return EA_PARAMS_STRIDE;
    if (grads_stride < P) return EA_GRADS_STRIDE;
    if (exp_avg_stride < P) return EA_EXP_AVG_STRIDE;
    if (exp_avg_sq_stride < P) return EA_EXP_AVG_SQ_STRIDE;
    return EA_OK;
}

// ---- the active-model mask (nic_ensemble_adam_prepare_active / _update_active) ------------------------------------------------------
// `active`: int32 [n_models] on the device, non-zero = the model takes this step; NULL = every model does.  The mask decides whether
// `ea_prepare` / `ea_update` (or the clipped pair) are CALLED for a model - their arithmetic is untouched - so a model that sits a
// step out keeps its counter, its products, its coef / clip rows and its rows of params and moments to the bit.  Its contents are
// device memory: the host can refuse the address only.
NIC_EA_FN bool ea_model_steps(const int32_t* active, int64_t m) { return active == nullptr || active[m] != 0; }
NIC_EA_FN int ea_check_active(const void* active) { return ((uintptr_t)active & 3) == 0 ? EA_OK : EA_ACTIVE; }
// one pair serves both steps: max_norm == NULL is the unclipped one (then clip and, for `prepare`, grads are NULL too)
NIC_EA_FN int ea_check_prepare_active(int n_models, int P, const void* hyper, const void* max_norm, const void* state, const void* coef,
                                      const void* grads, int64_t grads_stride, const void* clip, const void* active) {
    if (n_models < 1 || n_models > kEaMaxModels) return EA_MODELS;
    if (!hyper || !state || !coef) return EA_NULL;
    if ((max_norm != nullptr) != (clip != nullptr) || (max_norm != nullptr) != (grads != nullptr)) return EA_CLIP_TOGETHER;
    if (max_norm) {
        if (P < 1) return EA_COLUMNS;
        if (grads_stride < P) return EA_GRADS_STRIDE;
    }
    return ea_check_active(active);
}
NIC_EA_FN int ea_check_update_active(int n_models, int P, const void* params, int64_t params_stride, const void* grads, int64_t grads_stride,
                                     const void* exp_avg, int64_t exp_avg_stride, const void* exp_avg_sq, int64_t exp_avg_sq_stride,
                                     const void* coef, const void* active) {
    if (const int r = ea_check_update(n_models, P, params, params_stride, grads, grads_stride, exp_avg, exp_avg_stride, exp_avg_sq,
                                      exp_avg_sq_stride, coef))
        return r;
    return ea_check_active(active);
}

}  // namespace nic
