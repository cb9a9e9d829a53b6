// nic_ensemble_adam_prepare / nic_ensemble_adam_update: one Adam step for K models whose parameters, gradients and moments are
// rows of [K][stride >= P] buffers - two launches for all of them instead of K optimizers' launches (main_run.py:110's
// `torch.optim.Adam`, stepped by trainer.py:177's `optimizer.step()`).  The arithmetic is csrc/ensemble_adam_body.h's, which the host
// harness runs too: `prepare` is one thread per model in double, `update` one element per thread in float with plain coalesced
// loads and stores (K x P is a few tens of thousands of floats and the weights' row stride P is odd: launch latency bounds it).
// Built with -ffp-contract=off; float division and square root are the correctly rounded ones (hipcc's default).  Nothing here
// knows about layers.
// nic_ensemble_adam_prepare_clipped / _update_clipped: the same step with every model's total gradient norm clipped first
// (trainer.py:175-176's `clip_grad_norm_`), arithmetic in csrc/ensemble_clip_body.h - still two launches, further down.
#include "nic_common.h"
#include "ensemble_adam_body.h"
#include "ensemble_clip_body.h"

namespace {
constexpr int kT = nic::kEaThreads;

__global__ __launch_bounds__(kT) void ensemble_adam_prepare_kernel(int n_models, const double* __restrict__ hyper, nic::EaState* __restrict__ state,
                                                                   float* __restrict__ coef, const int32_t* __restrict__ active) {
    const int m = blockIdx.x * kT + threadIdx.x;
    if (m < n_models && nic::ea_model_steps(active, m)) nic::ea_prepare(hyper + (int64_t)m * nic::EA_HYPER_COUNT, state + m, coef + (int64_t)m * nic::EA_COEF_COUNT);
}

// grid (ceil(P / 256), K): columns at or past P of a row are neither read nor written
__global__ __launch_bounds__(kT) void ensemble_adam_update_kernel(int P, float* __restrict__ params, int64_t params_stride,
                                                                  const float* __restrict__ grads, int64_t grads_stride,
                                                                  float* __restrict__ exp_avg, int64_t exp_avg_stride,
                                                                  float* __restrict__ exp_avg_sq, int64_t exp_avg_sq_stride,
                                                                  const float* __restrict__ coef, const int32_t* __restrict__ active) {
    const int64_t m = blockIdx.y;
    if (!nic::ea_model_steps(active, m)) return;   // (wave-uniform: the model's rows are neither read nor written)
    const int col = blockIdx.x * kT + threadIdx.x;
    if (col >= P) return;
    nic::ea_update(params + m * params_stride + col, grads[m * grads_stride + col], exp_avg + m * exp_avg_stride + col,
                   exp_avg_sq + m * exp_avg_sq_stride + col, coef + m * nic::EA_COEF_COUNT);
}

// ---- the same step with every model's gradient norm clipped (csrc/ensemble_clip_body.h) -------------------------------------------
// grid K, one workgroup per model: thread i adds the squares of columns i, i + 256, ... of the model's gradient row in double, the
// 256 lane sums meet in LDS in the header's tree order, thread 0 finishes the model (norm, scale, then the unclipped prepare).
// Columns at or past P are never read.  No launch of its own for the norm and no atomics: the order of the additions is fixed.
__global__ __launch_bounds__(kT) void ensemble_adam_prepare_clipped_kernel(int P, const double* __restrict__ hyper,
                                                                           const double* __restrict__ max_norm,
                                                                           nic::EaState* __restrict__ state, float* __restrict__ coef,
                                                                           const float* __restrict__ grads, int64_t grads_stride,
                                                                           float* __restrict__ clip, const int32_t* __restrict__ active) {
    __shared__ double lanes[kT];
    const int64_t m = blockIdx.x;
    if (!nic::ea_model_steps(active, m)) return;   // (the whole workgroup, ahead of the barriers)
    const int lane = threadIdx.x;
    lanes[lane] = nic::ec_lane_sum(grads + m * grads_stride, P, lane);
    __syncthreads();
    for (int stride = kT / 2; stride >= 1; stride >>= 1) {
        if (lane < stride) nic::ec_combine(lanes, lane, stride);
        __syncthreads();
    }
    if (lane == 0)
        nic::ec_finish(lanes[0], max_norm[m], hyper + m * nic::EA_HYPER_COUNT, state + m, coef + m * nic::EA_COEF_COUNT,
                       clip + m * nic::EC_CLIP_COUNT);
}

// the update's grid and bounds; the gradient is scaled by the model's clip[EC_SCALE] on its way into the unchanged body
__global__ __launch_bounds__(kT) void ensemble_adam_update_clipped_kernel(int P, float* __restrict__ params, int64_t params_stride,
                                                                          const float* __restrict__ grads, int64_t grads_stride,
                                                                          float* __restrict__ exp_avg, int64_t exp_avg_stride,
                                                                          float* __restrict__ exp_avg_sq, int64_t exp_avg_sq_stride,
                                                                          const float* __restrict__ coef, const float* __restrict__ clip,
                                                                          const int32_t* __restrict__ active) {
    const int64_t m = blockIdx.y;
    if (!nic::ea_model_steps(active, m)) return;
    const int col = blockIdx.x * kT + threadIdx.x;
    if (col >= P) return;
    nic::ec_update(params + m * params_stride + col, grads[m * grads_stride + col], clip[m * nic::EC_CLIP_COUNT + nic::EC_SCALE],
                   exp_avg + m * exp_avg_stride + col, exp_avg_sq + m * exp_avg_sq_stride + col, coef + m * nic::EA_COEF_COUNT);
}
// the launches behind the entry points; `tag`: "" or ",active" (the recorded name of the existing entry points stays theirs)
int launch_prepare(int32_t n_models, int32_t P, const double* hyper, const double* max_norm, NicEnsembleAdamState* state, float* coef,
                   const float* grads, int64_t grads_stride, float* clip, const int32_t* active, const char* tag, void* stream, const char* who) {
    if (max_norm) {
        nic::note_kernelf("ensemble_adam_prepare_clipped<%d,models=%d%s>", P, n_models, tag);
        hipLaunchKernelGGL(ensemble_adam_prepare_clipped_kernel, dim3(n_models), dim3(kT), 0, nic::as_stream(stream), P, hyper, max_norm, state,
                           coef, grads, grads_stride, clip, active);
    } else {
        nic::note_kernelf("ensemble_adam_prepare<models=%d%s>", n_models, tag);
        hipLaunchKernelGGL(ensemble_adam_prepare_kernel, dim3(nic::ceil_div(n_models, kT)), dim3(kT), 0, nic::as_stream(stream), n_models, hyper,
                           state, coef, active);
    }
    return nic::check_launch(who);
}

int launch_update(int32_t n_models, int32_t P, float* params, int64_t params_stride, const float* grads, int64_t grads_stride, float* exp_avg,
                  int64_t exp_avg_stride, float* exp_avg_sq, int64_t exp_avg_sq_stride, const float* coef, const float* clip,
                  const int32_t* active, const char* tag, void* stream, const char* who) {
    const dim3 grid(nic::ceil_div(P, kT), n_models);
    if (clip) {
        nic::note_kernelf("ensemble_adam_update_clipped<%d,models=%d%s>", P, n_models, tag);
        hipLaunchKernelGGL(ensemble_adam_update_clipped_kernel, grid, dim3(kT), 0, nic::as_stream(stream), P, params, params_stride, grads,
                           grads_stride, exp_avg, exp_avg_stride, exp_avg_sq, exp_avg_sq_stride, coef, clip, active);
    } else {
        nic::note_kernelf("ensemble_adam_update<%d,models=%d%s>", P, n_models, tag);
        hipLaunchKernelGGL(ensemble_adam_update_kernel, grid, dim3(kT), 0, nic::as_stream(stream), P, params, params_stride, grads,
                           grads_stride, exp_avg, exp_avg_stride, exp_avg_sq, exp_avg_sq_stride, coef, active);
    }
    return nic::check_launch(who);
}
}  // namespace

extern "C" {

int nic_ensemble_adam_prepare(int32_t n_models, const double* hyper, NicEnsembleAdamState* state, float* coef, void* stream) {
    const int why = nic::ea_check_prepare(n_models, hyper, state, coef);
    NIC_REQUIRE(why == 0, "nic_ensemble_adam_prepare: %s (%d models)", nic::ea_reason(why), n_models);
    return launch_prepare(n_models, 0, hyper, nullptr, state, coef, nullptr, 0, nullptr, nullptr, "", stream, "nic_ensemble_adam_prepare");
}

int nic_ensemble_adam_update(int32_t n_models, int32_t P, float* params, int64_t params_stride, const float* grads, int64_t grads_stride,
                             float* exp_avg, int64_t exp_avg_stride, float* exp_avg_sq, int64_t exp_avg_sq_stride, const float* coef,
                             void* stream) {
    const int why = nic::ea_check_update(n_models, P, params, params_stride, grads, grads_stride, exp_avg, exp_avg_stride, exp_avg_sq,
                                         exp_avg_sq_stride, coef);
    NIC_REQUIRE(why == 0, "nic_ensemble_adam_update: %s (%d models, P = %d, strides %lld %lld %lld %lld)", nic::ea_reason(why), n_models, P,
                (long long)params_stride, (long long)grads_stride, (long long)exp_avg_stride, (long long)exp_avg_sq_stride);
    return launch_update(n_models, P, params, params_stride, grads, grads_stride, exp_avg, exp_avg_stride, exp_avg_sq, exp_avg_sq_stride, coef,
                         nullptr, nullptr, "", stream, "nic_ensemble_adam_update");
}

int nic_ensemble_adam_prepare_clipped(int32_t n_models, int32_t P, const double* hyper, const double* max_norm, NicEnsembleAdamState* state,
                                      float* coef, const float* grads, int64_t grads_stride, float* clip, void* stream) {
    const int why = nic::ec_check_prepare(n_models, P, hyper, max_norm, state, coef, grads, grads_stride, clip);
    NIC_REQUIRE(why == 0, "nic_ensemble_adam_prepare_clipped: %s (%d models, P = %d, gradient stride %lld)", nic::ea_reason(why), n_models, P,
                (long long)grads_stride);
    return launch_prepare(n_models, P, hyper, max_norm, state, coef, grads, grads_stride, clip, nullptr, "", stream,
                          "nic_ensemble_adam_prepare_clipped");
}

int nic_ensemble_adam_update_clipped(int32_t n_models, int32_t P, float* params, int64_t params_stride, const float* grads,
                                     int64_t grads_stride, float* exp_avg, int64_t exp_avg_stride, float* exp_avg_sq,
                                     int64_t exp_avg_sq_stride, const float* coef, const float* clip, void* stream) {
    const int why = nic::ec_check_update(n_models, P, params, params_stride, grads, grads_stride, exp_avg, exp_avg_stride, exp_avg_sq,
                                         exp_avg_sq_stride, coef, clip);
    NIC_REQUIRE(why == 0, "nic_ensemble_adam_update_clipped: %s (%d models, P = %d, strides %lld %lld %lld %lld)", nic::ea_reason(why), n_models,
                P, (long long)params_stride, (long long)grads_stride, (long long)exp_avg_stride, (long long)exp_avg_sq_stride);
    return launch_update(n_models, P, params, params_stride, grads, grads_stride, exp_avg, exp_avg_stride, exp_avg_sq, exp_avg_sq_stride, coef,
                         clip, nullptr, "", stream, "nic_ensemble_adam_update_clipped");
}

/* either step under the active-model mask: max_norm / clip NULL is the unclipped pair, else the clipped one */
int nic_ensemble_adam_prepare_active(int32_t n_models, int32_t P, const double* hyper, const double* max_norm, NicEnsembleAdamState* state,
                                     float* coef, const float* grads, int64_t grads_stride, float* clip, const int32_t* active, void* stream) {
    const int why = nic::ea_check_prepare_active(n_models, P, hyper, max_norm, state, coef, grads, grads_stride, clip, active);
    NIC_REQUIRE(why == 0, "nic_ensemble_adam_prepare_active: %s (%d models, P = %d, gradient stride %lld)", nic::ea_reason(why), n_models, P,
                (long long)grads_stride);
    return launch_prepare(n_models, P, hyper, max_norm, state, coef, grads, grads_stride, clip, active, ",active", stream,
                          "nic_ensemble_adam_prepare_active");
}

int nic_ensemble_adam_update_active(int32_t n_models, int32_t P, float* params, int64_t params_stride, const float* grads,
                                    int64_t grads_stride, float* exp_avg, int64_t exp_avg_stride, float* exp_avg_sq,
                                    int64_t exp_avg_sq_stride, const float* coef, const float* clip, const int32_t* active, void* stream) {
    const int why = nic::ea_check_update_active(n_models, P, params, params_stride, grads, grads_stride, exp_avg, exp_avg_stride, exp_avg_sq,
                                                exp_avg_sq_stride, coef, active);
    NIC_REQUIRE(why == 0, "nic_ensemble_adam_update_active: %s (%d models, P = %d, strides %lld %lld %lld %lld)", nic::ea_reason(why), n_models,
                P, (long long)params_stride, (long long)grads_stride, (long long)exp_avg_stride, (long long)exp_avg_sq_stride);
    return launch_update(n_models, P, params, params_stride, grads, grads_stride, exp_avg, exp_avg_stride, exp_avg_sq, exp_avg_sq_stride, coef,
                         clip, active, ",active", stream, "nic_ensemble_adam_update_active");
}

}  // extern "C"
