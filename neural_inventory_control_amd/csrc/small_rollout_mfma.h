// Device helpers the 32- and the 16-scenario whole-horizon kernels share (small_rollout.hip, small_rollout16.hip).
#pragma once
#include <hip/hip_runtime.h>

#include "small_rollout_variants.h"

namespace nic {

// Shape specialisation.  The per-lane env step / head bodies (small_rollout_body.h) index the st[16] register array with offsets
// built from the descriptor's pipeline lengths; with those as run-time values every access is a 16-way select chain whose 64-bit
// lane masks live in (spilled) SGPRs - 4,100 instructions per period, a quarter of them v_readlane / s_nop spill traffic, on a
// kernel whose duration IS the instruction count of one wavefront (one wave per SIMD, T sequential periods).  The two chains the
// reference ships are therefore compiled with their structure as constants: overwriting the structural fields of the kernel's
// own copy of the descriptor lets constant propagation fold every offset, loop bound and select through the always-inline bodies.
// (SHAPE: SrShape of small_rollout_variants.h, whose sr_shape_of recognises on the host what is written here.)
template <int SHAPE>
__device__ __forceinline__ void sr_fix_shape(NicSmallRolloutDesc& d, int n_hidden) {
    d.n_hidden = n_hidden;
    if (SHAPE == SR_ONE_STORE) {
        d.Ws = 4; d.Ww = 0; d.We = 0; d.Wn = 0; d.E = 0; d.head = 0; d.F = 4; d.n_out = 1;
    } else if (SHAPE == SR_SERIAL) {
        d.Ws = 4; d.Ww = 3; d.We = 4; d.Wn = 1; d.E = 2; d.head = 1; d.F = 15; d.n_out = 4;
    }
}

// ELU of two pre-activations: the series of nic::expm1_neg with packed FP32 FMAs (v_pk_fma_f32: two elements per instruction; each
// component rounds exactly like the scalar fmaf chain, so the values are those of nic::elu1).  The activations are more than half of
// the forward kernels' instruction stream (48 per scenario-period).
typedef float f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void sr_elu_pair(float z0, float z1, float& out0, float& out1) {
    const f32x2 x = {z0, z1};
    f32x2 p = __builtin_elementwise_fma(x, (f32x2)(1.f / 720.f), (f32x2)(1.f / 120.f));
    p = __builtin_elementwise_fma(x, p, (f32x2)(1.f / 24.f));
    p = __builtin_elementwise_fma(x, p, (f32x2)(1.f / 6.f));
    p = __builtin_elementwise_fma(x, p, (f32x2)(0.5f));
    p = __builtin_elementwise_fma(x, p, (f32x2)(1.f));
    const f32x2 sp = x * p;
    const float e0 = __expf(x.x) - 1.f, e1 = __expf(x.y) - 1.f;
    const float n0 = x.x > -0.35f ? sp.x : e0, n1 = x.y > -0.35f ? sp.y : e1;
    out0 = x.x > 0.f ? x.x : n0;
    out1 = x.y > 0.f ? x.y : n1;
}

}  // namespace nic
