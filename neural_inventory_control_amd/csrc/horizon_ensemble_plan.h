// K data_driven policies in one whole-horizon launch pair (nic_horizon_rollout_ensemble_*): the size of ONE model's slice of every
// per-model buffer and the checks an ensemble request has to pass before anything is launched.  Plain C++ on stack values, for host
// and device - no HIP, no allocation (tests/horizon_ensemble_plan_harness.cpp compiles it with the host compiler alone).  The entry
// points and the Python layer (nic_horizon_rollout_ensemble_slices) take their numbers from HERE.
//
// Model m (grid y) runs the single-model kernels' instruction stream on buffers that start m x stride floats behind model 0's: the
// kernels add that once, at entry, as a 64-bit pointer advance, and every 32-bit element offset they form afterwards is an offset
// inside ONE model's slice - what check_offsets (csrc/horizon_rollout.hip) bounds is unchanged by the number of models.
#pragma once
#include <stdint.h>
#include "../../include/nic_rollout.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define NIC_HE_FN __host__ __device__ inline
#else
#define NIC_HE_FN inline
#endif

namespace nic {

constexpr int kHeMaxModels = 65535;   // grid y

// ---- slices: rows x the row stride the descriptor gives each buffer -----------------------------------------------------------------
NIC_HE_FN NicHorizonEnsembleSlices horizon_ensemble_slices(const NicHorizonDesc& d) {
    const NicEnvDims& D = d.io.dims;
    const int64_t S = D.n_stores, Wn = D.n_warehouses, nsup = Wn > 0 ? Wn : 1;
    const int64_t FD = S * D.store_slots + Wn * D.warehouse_slots, n_ord = S * nsup + Wn, hs = d.hist_stride;
    NicHorizonEnsembleSlices s;
    s.W1 = d.H1 * d.ldw1;
    s.W2 = d.H2 * d.ldw2;
    s.W3 = d.n_out * d.ldw3;
    s.b2 = d.H2;
    s.b3 = d.n_out;
    s.z1_obs = d.H1 * hs;
    s.rewards = (int64_t)d.T * D.ldb;
    s.state_final = FD * D.ldb;
    s.state_hist = FD * hs;
    s.h1_hist = d.H1 * hs;
    s.h2_hist = d.H2 * hs;
    s.logits_hist = d.n_out * hs;
    s.orders_hist = (n_ord + Wn) * hs;   // (the orders, then what every warehouse shipped)
    s.dz1 = d.H1 * hs;
    s.dz2 = d.H2 * hs;
    s.dz3 = d.n_out * hs;
    return s;
}

// ---- checks ----------------------------------------------------------------------------------------------------------------------
// what a request is refused for (0: accepted); horizon_ensemble_reason names them
enum HorizonEnsembleRefusal {
    HE_OK = 0, HE_MODELS, HE_HEAD_MODE, HE_ROUND, HE_NEGATIVE, HE_W1, HE_W2, HE_W3, HE_B2, HE_B3, HE_Z1_OBS, HE_REWARDS, HE_FINAL,
    HE_STATE_HIST, HE_H1_HIST, HE_H2_HIST, HE_LOGITS_HIST, HE_ORDERS_HIST, HE_DZ1, HE_DZ2, HE_DZ3, HE_ALIGN,
};
NIC_HE_FN const char* horizon_ensemble_reason(int r) {
    switch (r) {
        case HE_OK: return "accepted";
        case HE_MODELS: return "n_models must be 1..65535";
        case HE_HEAD_MODE: return "only head_mode 0 (the MLP) has an ensemble form: a tape has no weights";
        case HE_ROUND: return "rounded orders have no gradient (evaluation only)";
        case HE_NEGATIVE: return "negative stride";
        case HE_W1: return "W1 stride shorter than H1 * ldw1";
        case HE_W2: return "W2 stride shorter than H2 * ldw2";
        case HE_W3: return "W3 stride shorter than n_out * ldw3";
        case HE_B2: return "b2 stride shorter than H2";
        case HE_B3: return "b3 stride shorter than n_out";
        case HE_Z1_OBS: return "z1_obs stride shorter than H1 * hist_stride";
        case HE_REWARDS: return "rewards stride shorter than T * ldb";
        case HE_FINAL: return "final-state stride shorter than the state rows x ldb";
        case HE_STATE_HIST: return "state-history stride shorter than its slice";
        case HE_H1_HIST: return "h1-history stride shorter than its slice";
        case HE_H2_HIST: return "h2-history stride shorter than its slice";
        case HE_LOGITS_HIST: return "logits-history stride shorter than its slice";
        case HE_ORDERS_HIST: return "orders-history stride shorter than its slice";
        case HE_DZ1: return "dz1 stride shorter than its slice";
        case HE_DZ2: return "dz2 stride shorter than its slice";
        case HE_DZ3: return "dz3 stride shorter than its slice";
        case HE_ALIGN: return "the strides of z1_obs, the rewards, the final state, the histories and the dz buffers must be multiples of 4 floats";
        default: return "?";
    }
}
NIC_HE_FN int horizon_ensemble_check_common(const NicHorizonDesc& d, const NicHorizonEnsemble& e, const NicHorizonEnsembleSlices& s) {
    if (e.n_models < 1 || e.n_models > kHeMaxModels) return HE_MODELS;
    if (d.head_mode != 0) return HE_HEAD_MODE;
    const int64_t all[16] = {e.W1, e.W2, e.W3, e.b2, e.b3, e.z1_obs, e.rewards, e.state_final, e.state_hist, e.h1_hist, e.h2_hist,
                             e.logits_hist, e.orders_hist, e.dz1, e.dz2, e.dz3};
    for (int i = 0; i < 16; ++i)
        if (all[i] < 0) return HE_NEGATIVE;
    if (e.W1 < s.W1) return HE_W1;
    if (e.W2 < s.W2) return HE_W2;
    if (e.W3 < s.W3) return HE_W3;
    if (e.b2 < s.b2) return HE_B2;
    if (e.b3 < s.b3) return HE_B3;
    return HE_OK;
}
// The kernels themselves read and write dwords; the 16-byte rule is for what is done with a model's slice next: nic_linear_fwd /
// nic_linear_wgrad and the cost reduction take each slice as a buffer of its own and load it with 16-byte accesses, so a slice must
// start on 16 bytes when model 0's does.  Weight strides are free (scalar reads).
NIC_HE_FN bool horizon_ensemble_aligned(int64_t stride) { return stride % 4 == 0; }
// forward: `with_final` / `with_history`: state_final / the five history buffers are passed
NIC_HE_FN int horizon_ensemble_check_fwd(const NicHorizonDesc& d, const NicHorizonEnsemble& e, const NicHorizonEnsembleSlices& s,
                                         bool with_final, bool with_history) {
    if (int r = horizon_ensemble_check_common(d, e, s)) return r;
    if (e.z1_obs < s.z1_obs) return HE_Z1_OBS;
    if (e.rewards < s.rewards) return HE_REWARDS;
    if (with_final && e.state_final < s.state_final) return HE_FINAL;
    if (with_history) {
        if (e.state_hist < s.state_hist) return HE_STATE_HIST;
        if (e.h1_hist < s.h1_hist) return HE_H1_HIST;
        if (e.h2_hist < s.h2_hist) return HE_H2_HIST;
        if (e.logits_hist < s.logits_hist) return HE_LOGITS_HIST;
        if (e.orders_hist < s.orders_hist) return HE_ORDERS_HIST;
    }
    if (!horizon_ensemble_aligned(e.z1_obs) || !horizon_ensemble_aligned(e.rewards)) return HE_ALIGN;
    if (with_final && !horizon_ensemble_aligned(e.state_final)) return HE_ALIGN;
    if (with_history && !(horizon_ensemble_aligned(e.state_hist) && horizon_ensemble_aligned(e.h1_hist) && horizon_ensemble_aligned(e.h2_hist) &&
                          horizon_ensemble_aligned(e.logits_hist) && horizon_ensemble_aligned(e.orders_hist)))
        return HE_ALIGN;
    return HE_OK;
}
NIC_HE_FN int horizon_ensemble_check_bwd(const NicHorizonDesc& d, const NicHorizonEnsemble& e, const NicHorizonEnsembleSlices& s) {
    if (int r = horizon_ensemble_check_common(d, e, s)) return r;
    if (d.round_orders) return HE_ROUND;
    if (e.state_hist < s.state_hist) return HE_STATE_HIST;
    if (e.h1_hist < s.h1_hist) return HE_H1_HIST;
    if (e.h2_hist < s.h2_hist) return HE_H2_HIST;
    if (e.logits_hist < s.logits_hist) return HE_LOGITS_HIST;
    if (e.orders_hist < s.orders_hist) return HE_ORDERS_HIST;
    if (e.dz1 < s.dz1) return HE_DZ1;
    if (e.dz2 < s.dz2) return HE_DZ2;
    if (e.dz3 < s.dz3) return HE_DZ3;
    if (!(horizon_ensemble_aligned(e.state_hist) && horizon_ensemble_aligned(e.h1_hist) && horizon_ensemble_aligned(e.h2_hist) &&
          horizon_ensemble_aligned(e.logits_hist) && horizon_ensemble_aligned(e.orders_hist) && horizon_ensemble_aligned(e.dz1) &&
          horizon_ensemble_aligned(e.dz2) && horizon_ensemble_aligned(e.dz3)))
        return HE_ALIGN;
    return HE_OK;
}

// ---- the kernels' side: model m's pointer advance ------------------------------------------------------------------------------
NIC_HE_FN int64_t horizon_model_offset(uint32_t model, int64_t stride) { return (int64_t)model * stride; }

}  // namespace nic
