// K small policies in one launch (nic_small_rollout_ensemble_*): the size of ONE model's slice of every buffer, the plan of the
// two-launch reduction (small_reduce.hip) and the checks an ensemble request has to pass before anything is launched.  Plain C++ on
// stack values, for host and device - no HIP, no allocation (tests/small_ensemble_plan_harness.cpp compiles it with the host
// compiler alone).  The entry points and the Python layer (nic_small_rollout_ensemble_slices) take their numbers from HERE.
#pragma once
#include <stdint.h>
#include "../../include/nic_rollout.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define NIC_SE_FN __host__ __device__ inline
#else
#define NIC_SE_FN inline
#endif

namespace nic {

constexpr int kSeMaxModels = 65535;   // grid y

// ---- the reduction's plan (one model): column chunks x row groups of the slab, blocks of the costs ------------------------------
constexpr int kSrReduceThreads = 256;     // threads per workgroup = columns per chunk
constexpr int kSrReduceMaxGroups = 64;    // row groups of the slab
constexpr int kSrReduceRewardBlocks = 256;
struct SrReducePlan { int cc, rg, rows_per_group, nb; };
NIC_SE_FN SrReducePlan sr_reduce_plan(int n_rows, int P, int64_t n_reward_elems) {
    SrReducePlan p;
    p.cc = P > 0 && n_rows > 0 ? (P + kSrReduceThreads - 1) / kSrReduceThreads : 0;
    p.rg = p.cc ? (n_rows < kSrReduceMaxGroups ? n_rows : kSrReduceMaxGroups) : 0;
    p.rows_per_group = p.rg ? (n_rows + p.rg - 1) / p.rg : 0;
    if (p.rg) p.rg = (n_rows + p.rows_per_group - 1) / p.rows_per_group;   // (no empty groups)
    const int64_t n4 = n_reward_elems / 4, blocks = (n4 + kSrReduceThreads - 1) / kSrReduceThreads;
    p.nb = n4 > 0 ? (int)(blocks < kSrReduceRewardBlocks ? blocks : kSrReduceRewardBlocks) : 0;
    return p;
}
NIC_SE_FN int sr_reduce_scratch(int n_rows, int P, int64_t n_reward_elems) {
    const SrReducePlan p = sr_reduce_plan(n_rows, P, n_reward_elems);
    return p.cc * p.rg * kSrReduceThreads + 2 * p.nb + 4;   // (<= 64 row groups x the column chunks x 256 floats)
}

// ---- slices ----------------------------------------------------------------------------------------------------------------------
NIC_SE_FN int sr_packed_count(int F, int n_hidden, int n_out) {
    return (NIC_SR_HIDDEN * F + NIC_SR_HIDDEN) + (n_hidden - 1) * (NIC_SR_HIDDEN * NIC_SR_HIDDEN + NIC_SR_HIDDEN) + (n_out * NIC_SR_HIDDEN + n_out);
}
// lane_width: 16 or 32 scenarios per wavefront (what NicSmallRolloutDesc::lane_scenarios resolves to)
NIC_SE_FN NicSmallEnsembleSlices small_ensemble_slices(int n_scenarios, int ldb, int T, int F, int n_hidden, int n_out, int lane_width) {
    NicSmallEnsembleSlices s;
    const int64_t tl = (int64_t)T * ldb;
    const bool w16 = lane_width == 16;
    s.weights = sr_packed_count(F, n_hidden, n_out);
    s.rewards = tl;
    s.final_state = (int64_t)F * ldb;
    s.states = (int64_t)(w16 ? NIC_SR16_STATE_ROWS(F) : F) * tl;
    s.hidden = (int64_t)NIC_SR_HIDDEN * n_hidden * tl;
    s.logits = (int64_t)(w16 ? NIC_SR16_LOGIT_ROWS(n_out) : n_out) * tl;
    s.slab_rows = (n_scenarios + lane_width - 1) / lane_width;
    s.slab_row_stride = (s.weights + 3) / 4 * 4;
    s.slab = s.slab_rows * s.slab_row_stride;
    s.grad = s.slab_row_stride;
    s.scratch = sr_reduce_scratch((int)s.slab_rows, (int)s.slab_row_stride, tl);
    return s;
}

// ---- checks ----------------------------------------------------------------------------------------------------------------------
// what a request is refused for (0: accepted); small_ensemble_reason names them
enum SmallEnsembleRefusal {
    SE_OK = 0, SE_MODELS, SE_WEIGHTS, SE_REWARDS, SE_FINAL, SE_STATES, SE_HIDDEN, SE_LOGITS, SE_SLAB_ROW, SE_SLAB, SE_GRAD, SE_SCRATCH,
    SE_ALIGN, SE_ACTIVE,
};
NIC_SE_FN const char* small_ensemble_reason(int r) {
    switch (r) {
        case SE_OK: return "accepted";
        case SE_MODELS: return "n_models must be 1..65535";
        case SE_WEIGHTS: return "weights stride shorter than the packed weights";
        case SE_REWARDS: return "rewards stride shorter than T * ldb";
        case SE_FINAL: return "final-state stride shorter than F * ldb";
        case SE_STATES: return "states-history stride shorter than its slice";
        case SE_HIDDEN: return "hidden-history stride shorter than its slice";
        case SE_LOGITS: return "logits-history stride shorter than its slice";
        case SE_SLAB_ROW: return "slab rows shorter than the packed weights";
        case SE_SLAB: return "slab stride shorter than rows x row stride";
        case SE_GRAD: return "grad stride shorter than the columns";
        case SE_SCRATCH: return "scratch stride shorter than the reduction's scratch";
        case SE_ALIGN: return "the strides of the rewards and the histories must be multiples of 4 floats";
        case SE_ACTIVE: return "the active mask must be NULL or 4-byte aligned";
        default: return "?";
    }
}
NIC_SE_FN int small_ensemble_check_models(const NicSmallEnsemble& e) { return e.n_models >= 1 && e.n_models <= kSeMaxModels ? SE_OK : SE_MODELS; }
// forward: `with_history`: the three history buffers are passed
NIC_SE_FN int small_ensemble_check_fwd(const NicSmallEnsemble& e, const NicSmallEnsembleSlices& s, bool with_history) {
    if (int r = small_ensemble_check_models(e)) return r;
    if (e.weights < s.weights) return SE_WEIGHTS;
    if (e.rewards < s.rewards) return SE_REWARDS;
    if (e.final_state < s.final_state) return SE_FINAL;
    if (e.rewards % 4 != 0) return SE_ALIGN;
    if (with_history) {
        if (e.states < s.states) return SE_STATES;
        if (e.hidden < s.hidden) return SE_HIDDEN;
        if (e.logits < s.logits) return SE_LOGITS;
        if (e.states % 4 != 0 || e.hidden % 4 != 0 || e.logits % 4 != 0) return SE_ALIGN;
    }
    return SE_OK;
}
NIC_SE_FN int small_ensemble_check_bwd(const NicSmallEnsemble& e, const NicSmallEnsembleSlices& s, int64_t slab_row_stride) {
    if (int r = small_ensemble_check_models(e)) return r;
    if (e.weights < s.weights) return SE_WEIGHTS;
    if (e.states < s.states) return SE_STATES;
    if (e.hidden < s.hidden) return SE_HIDDEN;
    if (e.logits < s.logits) return SE_LOGITS;
    if (e.states % 4 != 0 || e.hidden % 4 != 0 || e.logits % 4 != 0) return SE_ALIGN;
    if (slab_row_stride < s.weights) return SE_SLAB_ROW;
    if (e.slab < s.slab_rows * slab_row_stride) return SE_SLAB;
    return SE_OK;
}
// reduction of n_rows slab rows of P columns (with_slab) and / or n_reward_elems costs (with_rewards) per model
NIC_SE_FN int small_ensemble_check_reduce(const NicSmallEnsemble& e, bool with_slab, int n_rows, int64_t slab_row_stride, int P,
                                          bool with_rewards, int64_t n_reward_elems) {
    if (int r = small_ensemble_check_models(e)) return r;
    if (with_slab) {
        if (slab_row_stride < P) return SE_SLAB_ROW;
        if (e.slab < (int64_t)n_rows * slab_row_stride) return SE_SLAB;
        if (e.grad < P) return SE_GRAD;
    }
    if (with_rewards) {
        if (e.rewards < n_reward_elems) return SE_REWARDS;
        if (e.rewards % 4 != 0) return SE_ALIGN;
    }
    if (e.scratch < sr_reduce_scratch(with_slab ? n_rows : 0, with_slab ? P : 0, with_rewards ? n_reward_elems : 0)) return SE_SCRATCH;
    return SE_OK;
}

// ---- the active-model mask (nic_small_rollout_*_active) ---------------------------------------------------------------------------
// `active`: int32 [n_models] on the device, non-zero = the model runs; NULL = every model runs.  A workgroup of a model whose
// entry is zero returns before its first load or store, so no byte of that model's slices is read or written.  The mask's CONTENTS
// are device memory the host cannot read before the launch: what a request can be refused for is its address alone.
NIC_SE_FN int small_ensemble_check_active(const void* active) { return ((uintptr_t)active & 3) == 0 ? SE_OK : SE_ACTIVE; }
// what every K-model kernel asks at entry (m: its grid row; one scalar load and a branch)
NIC_SE_FN bool small_ensemble_model_runs(const int32_t* active, uint32_t m) { return active == nullptr || active[m] != 0; }

// ---- I problem instances (nic_small_rollout_instances_*) --------------------------------------------------------------------------
// The K models are I instances x R replicas: model m (grid y, as in every ensemble launch) reads instance m / R's demand trace,
// initial state and tables, each `instance x stride` floats behind instance 0's (stride 0: shared).  The kernels get m / R from one
// scalar multiply and shift by a constant the launcher computes: for m, R < 2^16, (m * ceil(2^32 / R)) >> 32 == m / R exactly (the
// constant times R exceeds 2^32 by less than R <= 2^16, so the product's error stays below one unit of the quotient).
// DECISION: the instance is NOT a third grid dimension.  Enabling the workgroup-id-z register moved the register allocation of the
// serial 32-scenario forward from 188 to 206 VGPRs (two wavefronts per SIMD -> one) although the value is dead after entry; the
// multiply-shift leaves every compiled-in instantiation at its registers (DESIGN.md records the figures).
constexpr int kSiTables = 8;   // underage, holding, lead, wh_holding, wh_lead, wh_edge, ech_holding, ech_lead (the descriptor's order)
NIC_SE_FN int small_instance_replicas(int n_models, int n_instances) { return n_models / n_instances; }
NIC_SE_FN uint64_t small_instance_magic(int replicas) { return ((1ull << 32) + (uint64_t)replicas - 1) / (uint64_t)replicas; }
NIC_SE_FN uint32_t small_instance_of(uint32_t model, uint64_t magic) { return (uint32_t)(((uint64_t)model * magic) >> 32); }
NIC_SE_FN int64_t small_instance_offset(uint32_t instance, int64_t stride) { return (int64_t)instance * stride; }
NIC_SE_FN NicSmallInstances small_instances_shared() { return NicSmallInstances{1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}; }
// table k's stride / the descriptor's table k
NIC_SE_FN int64_t small_instance_table_stride(const NicSmallInstances& in, int k) {
    const int64_t s[kSiTables] = {in.underage, in.holding, in.lead, in.wh_holding, in.wh_lead, in.wh_edge, in.ech_holding, in.ech_lead};
    return s[k];
}
NIC_SE_FN const float* small_instance_table_ptr(const NicSmallRolloutDesc& d, int k) {
    const float* p[kSiTables] = {d.underage.p, d.holding.p, d.lead.p, d.wh_holding.p, d.wh_lead.p, d.wh_edge.p, d.ech_holding.p, d.ech_lead.p};
    return p[k];
}
NIC_SE_FN const char* small_instance_table_name(int k) {
    const char* n[kSiTables] = {"underage", "holding", "lead", "wh_holding", "wh_lead", "wh_edge", "ech_holding", "ech_lead"};
    return n[k];
}
// the descriptor's eight tables <- instance `instance`'s (a NULL table has stride 0: it stays NULL); Strides: NicSmallInstances, or
// the kernels' view of one (the same ten strides)
template <class Strides>
NIC_SE_FN void small_instance_tables(NicSmallRolloutDesc& d, const Strides& in, uint32_t instance) {
    d.underage.p += small_instance_offset(instance, in.underage);
    d.holding.p += small_instance_offset(instance, in.holding);
    d.lead.p += small_instance_offset(instance, in.lead);
    d.wh_holding.p += small_instance_offset(instance, in.wh_holding);
    d.wh_lead.p += small_instance_offset(instance, in.wh_lead);
    d.wh_edge.p += small_instance_offset(instance, in.wh_edge);
    d.ech_holding.p += small_instance_offset(instance, in.ech_holding);
    d.ech_lead.p += small_instance_offset(instance, in.ech_lead);
}

enum SmallInstancesRefusal {
    SI_OK = 0, SI_COUNT, SI_DIVIDE, SI_GRID, SI_NEGATIVE, SI_DEMAND, SI_STATE0, SI_ALIGN, SI_NULL_TABLE,
};
NIC_SE_FN const char* small_instances_reason(int r) {
    switch (r) {
        case SI_OK: return "accepted";
        case SI_COUNT: return "n_instances must be at least 1";
        case SI_DIVIDE: return "n_instances must divide n_models";
        case SI_GRID: return "n_instances and the replicas per instance must be at most 65535";
        case SI_NEGATIVE: return "negative instance stride";
        case SI_DEMAND: return "demand stride shorter than (t0 + T) * ldb";
        case SI_STATE0: return "state0 stride shorter than F * ldb";
        case SI_ALIGN: return "the strides of demand and state0 must be multiples of 4 floats";
        case SI_NULL_TABLE: return "instance stride for a table whose pointer is NULL";
        default: return "?";
    }
}
// `d`: the request's descriptor (t0, T, ldb, F and which tables it has)
NIC_SE_FN int small_instances_check(const NicSmallInstances& in, int n_models, const NicSmallRolloutDesc& d) {
    if (in.n_instances < 1) return SI_COUNT;
    if (n_models % in.n_instances != 0) return SI_DIVIDE;
    if (in.n_instances > kSeMaxModels || small_instance_replicas(n_models, in.n_instances) > kSeMaxModels) return SI_GRID;
    if (in.demand < 0 || in.state0 < 0) return SI_NEGATIVE;
    for (int k = 0; k < kSiTables; ++k)
        if (small_instance_table_stride(in, k) < 0) return SI_NEGATIVE;
    if (in.demand != 0 && in.demand < ((int64_t)d.t0 + d.T) * d.ldb) return SI_DEMAND;
    if (in.state0 != 0 && in.state0 < (int64_t)d.F * d.ldb) return SI_STATE0;
    if (in.demand % 4 != 0 || in.state0 % 4 != 0) return SI_ALIGN;
    for (int k = 0; k < kSiTables; ++k)
        if (small_instance_table_stride(in, k) != 0 && small_instance_table_ptr(d, k) == nullptr) return SI_NULL_TABLE;
    return SI_OK;
}

}  // namespace nic
