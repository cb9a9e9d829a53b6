// Internal: launchers of the 16-scenarios-per-wavefront whole-horizon kernels (small_rollout16.hip), called by the C ABI entry
// points in small_rollout.hip (nic_small_rollout_fwd / nic_small_rollout_bwd_wgrad) when NicSmallRolloutDesc::lane_scenarios
// selects them.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "../../include/nic_rollout.h"
#include "nic_common.h"
#include "small_ensemble_plan.h"
#include "small_rollout_variants.h"

namespace nic {
// rows ([rows][T][ldb] floats) of the state / logit history of the 16-wide kernels: a scenario's slots are padded to whole 16-byte
// accesses (n_out = 1: one float, no padding)
__host__ __device__ inline int sr16_state_rows(int F) { return (F + 3) & ~3; }
__host__ __device__ inline int sr16_logit_rows(int n_out) { return n_out == 1 ? 1 : (n_out + 3) & ~3; }
// records the kernel name of a launch (small_rollout_variants.h words it); e: nullptr = one model; inst: nullptr = not one of the
// nic_small_rollout_instances_* entry points
inline void sr_note_kernel(SrRoute route, const NicSmallRolloutDesc& d, int shape, const NicSmallEnsemble* e,
                           const NicSmallInstances* inst = nullptr, bool active = false) {
    char name[160];
    sr_kernel_name(name, sizeof(name), route, sr_lane_width(d), d.n_hidden, shape, e ? e->n_models : 0, inst ? inst->n_instances : 0, active);
    note_kernelf("%s", name);
}
// What the ensemble instantiations take besides the single-model arguments: the per-model strides (Sr*Strides below) and the
// per-instance ones (all zero unless the launch came through nic_small_rollout_instances_*).  The single-model instantiations keep
// the per-model struct alone, which they do not read.
// SrInstanceStrides: a NicSmallInstances as the kernels take it - its ten strides at their offsets and, in the eight bytes of its
// count (which no kernel reads: the launcher turns the count into `magic`), the active-model mask.
// DECISION: the kernels that test the mask are instantiations of their own (template MASKED, launched by the *_active entry points
// only).  One scalar load and a branch at the entry of the existing ensemble instantiations moved the register allocation of
// kernels that never see a mask - the serial 32-scenario two-layer forward from 188 to 208 VGPRs (two wavefronts per SIMD -> one),
// as an early return, as an ended wavefront, with the pointer as a new argument or in the count's bytes alike.  With MASKED = false
// the field is not read and every kernel compiles to the instructions it had before the mask existed (DESIGN.md records the figures).
struct SrInstanceStrides {
    const int32_t* active;   // the active-model mask [K] (nic_small_rollout_*_active), NULL: every model runs
    int64_t demand, state0, underage, holding, lead, wh_holding, wh_lead, wh_edge, ech_holding, ech_lead;
};
static_assert(sizeof(SrInstanceStrides) == sizeof(NicSmallInstances) && offsetof(SrInstanceStrides, demand) == offsetof(NicSmallInstances, demand) &&
              offsetof(SrInstanceStrides, ech_lead) == offsetof(NicSmallInstances, ech_lead), "the kernels' view of NicSmallInstances");
template <class PerModel>
struct SrWithInstances : PerModel {
    SrInstanceStrides inst;
    uint64_t magic;   // small_instance_magic(models per instance): instance = small_instance_of(model, magic)
};
template <class PerModel, bool ENS>
using SrKernelStrides = std::conditional_t<ENS, SrWithInstances<PerModel>, PerModel>;
template <class PerModel>
inline SrWithInstances<PerModel> sr_with_instances(const PerModel& es, const NicSmallEnsemble* e, const NicSmallInstances* inst,
                                                   const int32_t* active = nullptr) {
    SrWithInstances<PerModel> out;
    static_cast<PerModel&>(out) = es;
    const NicSmallInstances in = inst ? *inst : small_instances_shared();
    out.inst = SrInstanceStrides{active, in.demand, in.state0, in.underage, in.holding, in.lead, in.wh_holding, in.wh_lead, in.wh_edge,
                                 in.ech_holding, in.ech_lead};
    out.magic = small_instance_magic(e ? small_instance_replicas(e->n_models, in.n_instances) : 1);
    return out;
}
// what the ensemble instantiations of the kernels take of a NicSmallEnsemble: floats between two models' slices of the buffers
// that kernel touches (the forward's history strides are zero when the histories are NULL: NULL + m x 0 stays NULL)
struct SrFwdStrides { int64_t weights, rewards, final_state, states, hidden, logits; };
struct SrBwdStrides { int64_t weights, states, hidden, logits, slab; };
inline SrFwdStrides sr_fwd_strides(const NicSmallEnsemble* e, bool with_history) {
    if (!e) return SrFwdStrides{0, 0, 0, 0, 0, 0};
    return SrFwdStrides{e->weights, e->rewards, e->final_state, with_history ? e->states : 0, with_history ? e->hidden : 0,
                        with_history ? e->logits : 0};
}
inline SrBwdStrides sr_bwd_strides(const NicSmallEnsemble* e) {
    return e ? SrBwdStrides{e->weights, e->states, e->hidden, e->logits, e->slab} : SrBwdStrides{0, 0, 0, 0, 0};
}
// e: nullptr = one model (the single-model instantiations), else K models, one grid row each (nic_small_rollout_ensemble_*), on
// inst's problem instances (nullptr: one, shared); mask: the _active entry points' (its `active` may be NULL), nullptr: every other
// entry point; false: no kernel for this n_hidden, nothing was launched
struct SrActive { const int32_t* active; };
bool small_rollout16_fwd(const NicSmallRolloutDesc& d, int shape, float* rewards, float* state_final, float* states_hist,
                         float* hidden_hist, float* logits_hist, hipStream_t s, const NicSmallEnsemble* e = nullptr,
                         const NicSmallInstances* inst = nullptr, const SrActive* mask = nullptr);
bool small_rollout16_bwd_wgrad(const NicSmallRolloutDesc& d, int shape, const float* states_hist, const float* hidden_hist,
                               const float* logits_hist, NicTable2 g_reward, float* slab, int64_t slab_stride, hipStream_t s,
                               const NicSmallEnsemble* e = nullptr, const NicSmallInstances* inst = nullptr, const SrActive* mask = nullptr);
}  // namespace nic
