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
    HE_STATE_HIST, HE_H1_HIST, HE_H2_HIST, HE_LOGITS_HIST, HE_ORDERS_HIST, HE_DZ1, HE_DZ2, HE_DZ3, HE_ALIGN, HE_ACTIVE,
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
        case HE_ACTIVE: return "the active mask must be NULL or 4-byte aligned";
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

// ---- the active-model mask (nic_horizon_rollout_ensemble_*_active / _instances_*_active) ------------------------------------------
// `active`: int32 [n_models] on the device, non-zero = the model runs; NULL = every model runs (the rule of
// csrc/small_ensemble_plan.h, whose _active entry points take NULL too).  A workgroup of a model whose entry is zero returns before
// its first pointer advance, load, store or barrier, so no byte of that model's slices is read or written.  The mask's CONTENTS
// are device memory the host cannot read before the launch: what a request can be refused for is its address alone.
NIC_HE_FN int horizon_ensemble_check_active(const void* active) { return ((uintptr_t)active & 3) == 0 ? HE_OK : HE_ACTIVE; }
// what the MASKED kernels ask at entry (m: the grid row; one scalar load and a branch)
NIC_HE_FN bool horizon_ensemble_model_runs(const int32_t* active, uint32_t m) { return active == nullptr || active[m] != 0; }

// ---- the kernels' side: model m's pointer advance ------------------------------------------------------------------------------
NIC_HE_FN int64_t horizon_model_offset(uint32_t model, int64_t stride) { return (int64_t)model * stride; }

// ---- I problem instances (nic_horizon_rollout_instances_*) -------------------------------------------------------------------------
// The K models are I instances x R replicas: model m (grid y, as in every ensemble launch) reads instance m / R's demand trace,
// initial state and the six tables hz_stage_tables stages, each `instance x stride` floats behind instance 0's (stride 0: shared).
// The advance is made once, at entry, beside the per-model one, as 64-bit pointer arithmetic: every 32-bit element offset formed
// afterwards is an offset inside ONE instance's slice, so check_offsets bounds what it bounds for one instance, whatever I is.
// The grid stays (x, K): the kernels get m / R from one scalar multiply and shift by a constant the launcher computes (the rule of
// csrc/small_ensemble_plan.h, whose third grid dimension cost the small forward 18 VGPRs): for m, R < 2^16,
// (m * ceil(2^32 / R)) >> 32 == m / R exactly.  blockIdx.y and the constant are scalars, so the instance index is wave-uniform
// and the advances stay on the scalar unit.
// The demand slice is (t0 + T) * S * ldb: neither kernel reads period t0 + T (the forward's last prefetch re-reads period
// t0 + T - 1, the backward fetches period t - 1 only while t > 0), so nothing of instance i + 1's trace is read for instance i.
constexpr int kHiTables = 6;   // underage, holding, lead_times, wh_holding, wh_lead_times, wh_edge_costs (NicEnvStepIO's order)
NIC_HE_FN int horizon_instance_replicas(int n_models, int n_instances) { return n_models / n_instances; }
NIC_HE_FN uint32_t horizon_instance_of(uint32_t model, uint32_t replicas) { return model / replicas; }   // the rule
NIC_HE_FN uint64_t horizon_instance_magic(int replicas) { return ((1ull << 32) + (uint64_t)replicas - 1) / (uint64_t)replicas; }
NIC_HE_FN uint32_t horizon_instance_by_magic(uint32_t model, uint64_t magic) { return (uint32_t)(((uint64_t)model * magic) >> 32); }   // what the kernels run
NIC_HE_FN int64_t horizon_instance_offset(uint32_t instance, int64_t stride) { return (int64_t)instance * stride; }
NIC_HE_FN NicHorizonInstances horizon_instances_shared() { return NicHorizonInstances{1, 0, 0, 0, 0, 0, 0, 0, 0, 0}; }
NIC_HE_FN int64_t horizon_instance_table_stride(const NicHorizonInstances& in, int k) {
    const int64_t s[kHiTables] = {in.underage, in.holding, in.lead, in.wh_holding, in.wh_lead, in.wh_edge};
    return s[k];
}
NIC_HE_FN const float* horizon_instance_table_ptr(const NicEnvStepIO& io, int k) {
    const float* p[kHiTables] = {io.underage.p, io.holding.p, io.lead_times.p, io.wh_holding.p, io.wh_lead_times.p, io.wh_edge_costs.p};
    return p[k];
}
// floats from a table's first element to one past the last the kernels address for `rows` locations (x `sups` suppliers) and B scenarios
NIC_HE_FN int64_t horizon_span(int64_t n, int64_t stride) { return (n - 1) * (stride < 0 ? -stride : stride); }
NIC_HE_FN int64_t horizon_table2_extent(const NicTable2& t, int rows, int B) {
    return rows > 0 ? horizon_span(rows, t.loc_stride) + horizon_span(B, t.scn_stride) + 1 : 0;
}
NIC_HE_FN int64_t horizon_table3_extent(const NicTable3& t, int rows, int sups, int B) {
    return rows > 0 ? horizon_span(rows, t.loc_stride) + horizon_span(sups, t.sup_stride) + horizon_span(B, t.scn_stride) + 1 : 0;
}
NIC_HE_FN int64_t horizon_instance_table_extent(const NicHorizonDesc& d, int k) {
    const NicEnvDims& D = d.io.dims;
    const int S = D.n_stores, Wn = D.n_warehouses, B = D.n_scenarios;
    switch (k) {
        case 0: return horizon_table2_extent(d.io.underage, S, B);
        case 1: return horizon_table2_extent(d.io.holding, S, B);
        case 2: return horizon_table3_extent(d.io.lead_times, S, Wn > 0 ? Wn : 1, B);
        case 3: return horizon_table2_extent(d.io.wh_holding, Wn, B);
        case 4: return horizon_table2_extent(d.io.wh_lead_times, Wn, B);
        default: return horizon_table2_extent(d.io.wh_edge_costs, Wn, B);
    }
}
NIC_HE_FN int64_t horizon_instance_demand_slice(const NicHorizonDesc& d) {
    return ((int64_t)d.t0 + d.T) * d.io.dims.n_stores * d.io.dims.ldb;
}
NIC_HE_FN int64_t horizon_instance_state0_slice(const NicHorizonDesc& d) {
    const NicEnvDims& D = d.io.dims;
    return ((int64_t)D.n_stores * D.store_slots + (int64_t)D.n_warehouses * D.warehouse_slots) * D.ldb;
}
// the six tables of the descriptor <- instance `instance`'s.  A NULL table has stride 0 (horizon_instances_check): it stays NULL.
NIC_HE_FN void horizon_instance_tables(NicEnvStepIO& io, const NicHorizonInstances& in, uint32_t instance) {
    io.underage.p += horizon_instance_offset(instance, in.underage);
    io.holding.p += horizon_instance_offset(instance, in.holding);
    io.lead_times.p += horizon_instance_offset(instance, in.lead);
    io.wh_holding.p += horizon_instance_offset(instance, in.wh_holding);
    io.wh_lead_times.p += horizon_instance_offset(instance, in.wh_lead);
    io.wh_edge_costs.p += horizon_instance_offset(instance, in.wh_edge);
}

enum HorizonInstancesRefusal {
    HI_OK = 0, HI_COUNT, HI_DIVIDE, HI_GRID, HI_NEGATIVE, HI_DEMAND, HI_STATE0, HI_ALIGN, HI_NULL_TABLE, HI_UNDERAGE, HI_HOLDING, HI_LEAD,
    HI_WH_HOLDING, HI_WH_LEAD, HI_WH_EDGE,
};
NIC_HE_FN const char* horizon_instances_reason(int r) {
    switch (r) {
        case HI_OK: return "accepted";
        case HI_COUNT: return "n_instances must be 1..65535";
        case HI_DIVIDE: return "n_instances must divide n_models";
        case HI_GRID: return "the replicas per instance must be at most 65535";
        case HI_NEGATIVE: return "negative instance stride";
        case HI_DEMAND: return "demand stride shorter than (t0 + T) * S * ldb";
        case HI_STATE0: return "state0 stride shorter than the state rows x ldb";
        case HI_ALIGN: return "the strides of demand and state0 must be multiples of 4 floats";
        case HI_NULL_TABLE: return "instance stride for a table whose pointer is NULL";
        case HI_UNDERAGE: return "underage stride shorter than the table";
        case HI_HOLDING: return "holding stride shorter than the table";
        case HI_LEAD: return "lead-time stride shorter than the table";
        case HI_WH_HOLDING: return "warehouse-holding stride shorter than the table";
        case HI_WH_LEAD: return "warehouse-lead-time stride shorter than the table";
        case HI_WH_EDGE: return "warehouse-edge-cost stride shorter than the table";
        default: return "?";
    }
}
// `d`: the request's descriptor (t0, T, the dims and the tables with their strides)
NIC_HE_FN int horizon_instances_check(const NicHorizonInstances& in, int n_models, const NicHorizonDesc& d) {
    if (in.n_instances < 1 || in.n_instances > kHeMaxModels) return HI_COUNT;
    if (n_models % in.n_instances != 0) return HI_DIVIDE;
    if (horizon_instance_replicas(n_models, in.n_instances) > kHeMaxModels) return HI_GRID;
    if (in.demand < 0 || in.state0 < 0) return HI_NEGATIVE;
    for (int k = 0; k < kHiTables; ++k)
        if (horizon_instance_table_stride(in, k) < 0) return HI_NEGATIVE;
    if (in.demand != 0 && in.demand < horizon_instance_demand_slice(d)) return HI_DEMAND;
    if (in.state0 != 0 && in.state0 < horizon_instance_state0_slice(d)) return HI_STATE0;
    if (in.demand % 4 != 0 || in.state0 % 4 != 0) return HI_ALIGN;
    for (int k = 0; k < kHiTables; ++k) {
        const int64_t stride = horizon_instance_table_stride(in, k);
        if (stride == 0) continue;
        if (horizon_instance_table_ptr(d.io, k) == nullptr) return HI_NULL_TABLE;
        if (stride < horizon_instance_table_extent(d, k)) return HI_UNDERAGE + k;
    }
    return HI_OK;
}

}  // namespace nic
