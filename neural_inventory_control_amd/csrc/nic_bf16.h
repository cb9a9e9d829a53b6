// FP32 -> bf16 conversion of the opt-in bf16 GEMMs (linear_bf16.hip).  One helper for host and device so that the rounding the
// kernels apply can be checked on the host bit for bit (tests/test_bf16_host.py compiles tests/bf16_convert_harness.cpp against it).
// A plain cast: round to nearest even, NaN stays NaN (a quiet NaN), subnormals kept.  On gfx950 the device form is
// v_cvt_pk_bf16_f32 (MI355X_MICROARCH.md, conversion row).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__HIP__)
#define NIC_BF16_HD __host__ __device__
#else
#define NIC_BF16_HD
#endif

NIC_BF16_HD inline uint16_t nic_f32_to_bf16_bits(float x) {
    const __bf16 b = static_cast<__bf16>(x);
    uint16_t u;
    __builtin_memcpy(&u, &b, sizeof(u));
    return u;
}

// two values packed as the low / high halves of one 32-bit word (lo = lower k of an MFMA operand fragment)
NIC_BF16_HD inline uint32_t nic_pack_bf16x2(float lo, float hi) {
    return (uint32_t)nic_f32_to_bf16_bits(lo) | ((uint32_t)nic_f32_to_bf16_bits(hi) << 16);
}
