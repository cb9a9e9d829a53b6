// The policy GEMMs for K models in one launch (nic_linear_fwd_models, nic_linear_wgrad_models, nic_wgrad_reduce_models,
// linear_mfma.hip): the checks a request has to pass before anything is launched, and its launch plan.  Plain C++ on stack values,
// for host and device - no HIP, no allocation, no environment; the compute-unit count is an argument
// (tests/linear_models_plan_harness.cpp compiles it with the host compiler alone).
//
// Model m (grid y) runs the single-model kernel's instruction stream on operands that start m x stride floats behind model 0's: a
// kernel adds that once, at entry, as a 64-bit pointer advance (linear_model_offset), and every offset it forms afterwards is an
// offset inside ONE model's slice.  The plan is the single-model entry point's plan for model 0's operands - the same calls into
// wx_plan.h / wgrad_plan.h, the same n_splits, the same operand-eligibility bits - so model m's outputs are the bits of
// nic_linear_fwd / nic_linear_wgrad / nic_wgrad_reduce called on its slice.  For that, every model's operands must pass the same
// 16-byte test as model 0's: the strides of W, X, Y, dY and the slab are multiples of 4 floats.  The bias, dW and db are read and
// written as scalars: their strides are free.
//
// Model forms exist for what the whole-horizon route of the data_driven policy asks for, and no more: forwards of N <= 64 output
// rows (the streamed kernels, the 64 x 128 and 32 x 128 LDS-DMA tiles, the guarded staged tiles of unaligned operands) and
// one-period weight gradients of N <= 128 (wgrad_small_kernel<1..4>, the four register-staged gemm_wgrad_kernel tiles, FAST and
// guarded).  A request whose plan picks another kernel is refused: LM_PLAN.
#pragma once
#include <stdint.h>

#include "wgrad_plan.h"
#include "wx_plan.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define NIC_LM_FN __host__ __device__ inline
#else
#define NIC_LM_FN inline
#endif

namespace nic {

constexpr int kLmMaxModels = 65535;   // grid y
constexpr int kLmFwdMaxRows = 64;     // forward: N <= 64 (horizon_rollout's MAX_HIDDEN)
constexpr int kLmWgradMaxRows = 128;  // weight gradient: N <= 128

// what a request is refused for (0: accepted); linear_models_reason names them
enum LinearModelsRefusal {
    LM_OK = 0, LM_MODELS, LM_NULL, LM_SIZES, LM_ACT, LM_LD, LM_POINTER_ALIGN, LM_SPLITS, LM_NEGATIVE,
    LM_Y_STRIDE, LM_SLAB_STRIDE, LM_DW_STRIDE, LM_DB_STRIDE,          // an output stride shorter than one model's slice
    LM_W_STRIDE, LM_BIAS_STRIDE, LM_X_STRIDE, LM_DY_STRIDE,           // an input stride that is neither allowed to be 0 nor >= the slice
    LM_ALIGN, LM_PLAN, LM_REFUSAL_END,                                // (the end of what a request without a mask can be refused for)
    LM_MASK = LM_REFUSAL_END, LM_ACTIVE_REFUSAL_END                   // the _active entry points' own
};
NIC_LM_FN const char* linear_models_reason(int r) {
    switch (r) {
        case LM_OK: return "accepted";
        case LM_MODELS: return "n_models must be 1..65535";
        case LM_NULL: return "null buffer";
        case LM_SIZES: return "bad N / K / leading dimension of the weights, the slab or dW";
        case LM_ACT: return "unknown activation";
        case LM_LD: return "ldb must be a multiple of 4 and >= n_scenarios > 0";
        case LM_POINTER_ALIGN: return "X / Y must be 16-byte aligned";
        case LM_SPLITS: return "n_splits must be >= 1";
        case LM_NEGATIVE: return "negative stride";
        case LM_Y_STRIDE: return "Y stride shorter than N * ldb";
        case LM_SLAB_STRIDE: return "slab stride shorter than n_splits * N * lds";
        case LM_DW_STRIDE: return "dW stride shorter than (N - 1) * lddw + K";
        case LM_DB_STRIDE: return "db stride shorter than N";
        case LM_W_STRIDE: return "W stride shorter than (N - 1) * ldw + K";
        case LM_BIAS_STRIDE: return "bias stride shorter than N";
        case LM_X_STRIDE: return "X stride shorter than K * ldb (0, one shared input, is taken by the forward only)";
        case LM_DY_STRIDE: return "dY stride shorter than N * ldb";
        case LM_ALIGN: return "the strides of W, X, Y, dY and the slab must be multiples of 4 floats";
        case LM_PLAN: return "the plan picks a kernel without a model form (forward: N <= 64; weight gradient: N <= 128, staged or small tiles)";
        case LM_MASK: return "the active mask must be NULL or 4-byte aligned";
        default: return "?";
    }
}

// ---- the active-model mask (nic_linear_fwd_models_active, nic_linear_wgrad_models_active, nic_wgrad_reduce_models_active) ---------
// `active`: int32 [n_models] on the device, non-zero = the model runs; NULL = every model runs (what the entry points without a
// mask pass).  A workgroup of a model whose entry is zero returns before its pointer advance: no byte of that model's operands is
// read or written.  Only the mask's address can be checked on the host (requests carry it as `active`, 0 = NULL).
NIC_LM_FN bool lm_mask_ok(uint64_t active) { return (active & 3) == 0; }
NIC_LM_FN bool linear_model_runs(const int32_t* active, uint32_t model) { return active == nullptr || active[model] != 0; }

// ---- the kernels' side: model m's pointer advance ------------------------------------------------------------------------------
NIC_LM_FN int64_t linear_model_offset(uint32_t model, int64_t stride) { return (int64_t)model * stride; }

// ---- requests: addresses as integers (only null-ness and the low 4 bits count), strides in floats --------------------------------
struct LmFwdRequest {
    uint64_t W, bias /* may be 0 */, X, Y;
    int64_t ldw, W_stride, bias_stride, X_stride, Y_stride;
    int N, K, n_scenarios, ldb, act, n_models;
    uint64_t active = 0;   // the mask's address (0: none)
};
struct LmWgradRequest {
    uint64_t dY, X, slab;
    int64_t dY_stride, X_stride, slab_stride, lds;
    int N, K, n_scenarios, ldb, n_splits, n_models;
    uint64_t active = 0;
};
struct LmReduceRequest {
    uint64_t slab, dW, db /* may be 0 */;
    int64_t slab_stride, lds, lddw, dW_stride, db_stride;
    int N, K, n_splits, n_models;
    uint64_t active = 0;
};

NIC_LM_FN bool lm_models_ok(int n_models) { return n_models >= 1 && n_models <= kLmMaxModels; }
NIC_LM_FN bool lm_ld_ok(int n_scenarios, int ldb) { return n_scenarios > 0 && ldb >= n_scenarios && ldb % 4 == 0; }

// ---- checks: the single-model entry point's argument errors, then the strides ----------------------------------------------------
NIC_LM_FN int linear_models_check_fwd(const LmFwdRequest& r) {
    if (!lm_models_ok(r.n_models)) return LM_MODELS;
    if (!r.W || !r.X || !r.Y) return LM_NULL;
    if (!(r.N > 0 && r.K > 0 && r.ldw >= r.K)) return LM_SIZES;
    if (r.act != NIC_ACT_NONE && r.act != NIC_ACT_ELU) return LM_ACT;
    if (!lm_ld_ok(r.n_scenarios, r.ldb)) return LM_LD;
    if ((r.X & 15) != 0 || (r.Y & 15) != 0) return LM_POINTER_ALIGN;
    if (r.W_stride < 0 || r.bias_stride < 0 || r.X_stride < 0 || r.Y_stride < 0) return LM_NEGATIVE;
    if (r.Y_stride < (int64_t)r.N * r.ldb) return LM_Y_STRIDE;
    if (r.W_stride < (int64_t)(r.N - 1) * r.ldw + r.K) return LM_W_STRIDE;
    if (r.bias && r.bias_stride < r.N) return LM_BIAS_STRIDE;
    if (r.X_stride != 0 && r.X_stride < (int64_t)r.K * r.ldb) return LM_X_STRIDE;
    if (r.W_stride % 4 != 0 || r.X_stride % 4 != 0 || r.Y_stride % 4 != 0) return LM_ALIGN;
    if (!lm_mask_ok(r.active)) return LM_MASK;
    return LM_OK;
}
NIC_LM_FN int linear_models_check_wgrad(const LmWgradRequest& r) {
    if (!lm_models_ok(r.n_models)) return LM_MODELS;
    if (!r.dY || !r.X || !r.slab) return LM_NULL;
    if (!(r.N > 0 && r.K > 0 && r.lds >= r.K + 1)) return LM_SIZES;
    if (r.n_splits < 1) return LM_SPLITS;
    if (!lm_ld_ok(r.n_scenarios, r.ldb)) return LM_LD;
    if (r.dY_stride < 0 || r.X_stride < 0 || r.slab_stride < 0) return LM_NEGATIVE;
    if (r.slab_stride < (int64_t)r.n_splits * r.N * r.lds) return LM_SLAB_STRIDE;
    if (r.dY_stride < (int64_t)r.N * r.ldb) return LM_DY_STRIDE;
    if (r.X_stride < (int64_t)r.K * r.ldb) return LM_X_STRIDE;
    if (r.dY_stride % 4 != 0 || r.X_stride % 4 != 0 || r.slab_stride % 4 != 0) return LM_ALIGN;
    if (!lm_mask_ok(r.active)) return LM_MASK;
    return LM_OK;
}
NIC_LM_FN int linear_models_check_reduce(const LmReduceRequest& r) {
    if (!lm_models_ok(r.n_models)) return LM_MODELS;
    if (!r.slab || !r.dW) return LM_NULL;
    if (!(r.N > 0 && r.K > 0 && r.lds >= r.K + 1 && r.lddw >= r.K)) return LM_SIZES;
    if (r.n_splits < 1) return LM_SPLITS;
    if (r.slab_stride < 0 || r.dW_stride < 0 || r.db_stride < 0) return LM_NEGATIVE;
    if (r.dW_stride < (int64_t)(r.N - 1) * r.lddw + r.K) return LM_DW_STRIDE;
    if (r.db && r.db_stride < r.N) return LM_DB_STRIDE;
    if (r.slab_stride < (int64_t)r.n_splits * r.N * r.lds) return LM_SLAB_STRIDE;
    if (r.slab_stride % 4 != 0) return LM_ALIGN;
    if (!lm_mask_ok(r.active)) return LM_MASK;
    return LM_OK;
}

// ---- plans: the single-model entry point's, for model 0's operands (host only: wx_plan.h and wgrad_plan.h are) -------------------
inline bool lm_wx_has_model_form(WxKernel k) {
    return k == WX_STREAM_1x2 || k == WX_STREAM_1x4 || k == WX_DMA_64x128 || k == WX_DMA_32x128 || k == WX_STAGED_64x128 ||
           k == WX_STAGED_32x256;
}
inline bool lm_wgrad_has_model_form(WgradTile t) { return t <= WG_SMALL_4 || t >= WG_STAGED_128x128; }

// nic_linear_fwd's plan: operands = nic_linear_fwd's eligibility bit, n_scenarios rounded up to 4 columns
struct LmFwdPlan { int refusal; bool operands; WxPlan plan; };
inline LmFwdPlan linear_models_fwd_plan(const LmFwdRequest& r, int cus, WxForce force = {}) {
    LmFwdPlan out = {linear_models_check_fwd(r), false, {WX_STREAM_1x2, 0}};
    if (out.refusal) return out;
    out.operands = wx_operands(r.W | r.X, r.ldw, r.ldb, r.N, r.K);
    out.plan = wx_plan(r.N, r.K, (r.n_scenarios + 3) / 4 * 4, out.operands, cus, force);
    if (r.N > kLmFwdMaxRows || !lm_wx_has_model_form(out.plan.kernel)) out.refusal = LM_PLAN;
    return out;
}
// nic_linear_wgrad's plan (WG_ONE_PERIOD: one launch of plan.tile_single over plan.slots slab slots)
struct LmWgradPlan { int refusal; WgradOperands operands; WgradPlan plan; };
inline LmWgradPlan linear_models_wgrad_plan(const LmWgradRequest& r, bool force_staged = false) {
    LmWgradPlan out = {linear_models_check_wgrad(r), {false, false}, {}};
    if (out.refusal) return out;
    out.operands = wgrad_operands(r.dY | r.X, r.slab, r.ldb, r.lds, r.N, r.K);
    out.plan = wgrad_plan(WG_ONE_PERIOD, r.N, r.K, r.n_scenarios, 1, r.n_splits, out.operands, force_staged);
    if (r.N > kLmWgradMaxRows || !lm_wgrad_has_model_form(wgrad_launch(out.plan, 1, 0).tile)) out.refusal = LM_PLAN;
    return out;
}
// nic_wgrad_reduce's choice between its two kernels
inline bool wgrad_reduce_wide(int n_splits, int N, int K) { return n_splits >= 128 && (int64_t)N * (K + 1) <= 65536; }

}  // namespace nic
