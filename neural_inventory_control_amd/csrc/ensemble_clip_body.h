// Gradient-norm clipping inside the Adam step of K models (nic_ensemble_adam_prepare_clipped / _update_clipped,
// csrc/ensemble_adam.hip): trainer.py:175-176's `clip_grad_norm_(model.parameters(), max_norm)` per model, between the gradients
// and csrc/ensemble_adam_body.h's update.  Same rules as that header: plain C++ on values the caller hands in, for host and
// device - no HIP, no allocation (tests/ensemble_clip_harness.cpp compiles it with the host compiler alone and is the referee of
// the kernels, bit for bit).
//
// Per model, before `ea_prepare`: the sum of squares of the row's P live gradient columns in DOUBLE (a float squared is exact in
// double, so only the additions round), in an order fixed HERE: lane i of kEaThreads adds columns i, i + 256, ... in increasing
// order (`ec_lane_sum`), then the 256 lane sums are combined by a pairwise tree, strides 128, 64, ... 1, lane i taking lane
// i + stride (`ec_combine`).  `ec_row_sum` is that order on one thread; the kernel runs the same two pieces with one lane a thread
// and the lane sums in LDS.  `ec_finish`: norm = sqrt(sum), scale = max_norm == +inf ? 1 : min(1, max_norm / (norm + 1e-6)) in
// double (torch's `clip_grad_norm_`), rounded to float once; clip = {scale, (float)norm}; then the unchanged `ea_prepare`.  A
// non-finite gradient gives a non-finite norm and scale, which propagate as in torch with error_if_nonfinite=False.
// Per element: `ea_update` on g * scale (float; the units are built with -ffp-contract=off, so with scale == 1.0f the result is
// the unclipped update's bits).
//
// Sized for the ensembles' rows, P of 10^3 to 10^5: one workgroup walks a row (4 to 400 columns a lane), which keeps the norm
// inside the prepare launch - no launch of its own, no atomics.  Rows of many millions of columns would want the row split over
// workgroups; nothing here does that.
#pragma once
#include "ensemble_adam_body.h"

namespace nic {

// one model's row of the clip table (floats): what the update reads, and the norm `clip_grad_norm_` returns
enum EcClip { EC_SCALE = 0, EC_NORM, EC_CLIP_COUNT };
constexpr double kEcNormEps = 1e-6;   // torch.nn.utils.clip_grad_norm_'s

// ---- per model: the sum of squares, in the order every build of it keeps -----------------------------------------------------------
// (kEcLoads columns are loaded before the first of them is added, so that a lane's loads do not wait for one another; the additions
// keep their order)
constexpr int kEcLoads = 8;
NIC_EA_FN double ec_lane_sum(const float* g, int P, int lane) {
    double s = 0.0;
    int64_t c = lane;
    for (; c + (kEcLoads - 1) * kEaThreads < P; c += kEcLoads * kEaThreads) {
        float x[kEcLoads];
        for (int u = 0; u < kEcLoads; ++u) x[u] = g[c + u * kEaThreads];
        for (int u = 0; u < kEcLoads; ++u) s = s + (double)x[u] * (double)x[u];
    }
    for (; c < P; c += kEaThreads) s = s + (double)g[c] * (double)g[c];
    return s;
}
// one node of the tree: callers run strides kEaThreads / 2, ... 1, every lane < stride, all of a stride before the next
NIC_EA_FN void ec_combine(double* lanes, int lane, int stride) { lanes[lane] = lanes[lane] + lanes[lane + stride]; }

NIC_EA_FN double ec_row_sum(const float* g, int P) {
    double lanes[kEaThreads];
    for (int i = 0; i < kEaThreads; ++i) lanes[i] = ec_lane_sum(g, P, i);
    for (int stride = kEaThreads / 2; stride >= 1; stride >>= 1)
        for (int i = 0; i < stride; ++i) ec_combine(lanes, i, stride);
    return lanes[0];
}

// ---- per model: norm, scale, then the step's coefficients -------------------------------------------------------------------------
NIC_EA_FN void ec_finish(double sum, double max_norm, const double* hyper, EaState* state, float* coef, float* clip) {
    const double norm = sqrt(sum);
    double c = 1.0;
    if (!(max_norm == (double)INFINITY)) {
        c = max_norm / (norm + kEcNormEps);
        if (c > 1.0) c = 1.0;   // (a NaN stays one)
    }
    clip[EC_SCALE] = (float)c;
    clip[EC_NORM] = (float)norm;
    ea_prepare(hyper, state, coef);
}

// ---- per element ------------------------------------------------------------------------------------------------------------------
NIC_EA_FN void ec_update(float* p, float g, float scale, float* exp_avg, float* exp_avg_sq, const float* coef) {
    ea_update(p, g * scale, exp_avg, exp_avg_sq, coef);
}

// ---- checks (refusals and reasons are ensemble_adam_body.h's: EaRefusal, ea_reason) ------------------------------------------------
NIC_EA_FN int ec_check_prepare(int n_models, int P, const void* hyper, const void* max_norm, const void* state, const void* coef,
                               const void* grads, int64_t grads_stride, const void* clip) {
    if (n_models < 1 || n_models > kEaMaxModels) return EA_MODELS;
    if (P < 1) return EA_COLUMNS;
    if (!hyper || !max_norm || !state || !coef || !grads || !clip) return EA_NULL;
    if (grads_stride < P) return EA_GRADS_STRIDE;
    return EA_OK;
}
NIC_EA_FN int ec_check_update(int n_models, int P, const void* params, int64_t params_stride, const void* grads, int64_t grads_stride,
                              const void* exp_avg, int64_t exp_avg_stride, const void* exp_avg_sq, int64_t exp_avg_sq_stride,
                              const void* coef, const void* clip) {
    if (const int r = ea_check_update(n_models, P, params, params_stride, grads, grads_stride, exp_avg, exp_avg_stride, exp_avg_sq,
                                      exp_avg_sq_stride, coef))
        return r;
    if (!clip) return EA_NULL;
    return EA_OK;
}

}  // namespace nic
