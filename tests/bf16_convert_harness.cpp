// Host build of the kernels' FP32 -> bf16 conversion (csrc/nic_bf16.h) for tests/test_bf16_host.py: compiled with the host
// compiler into a small shared library and called through ctypes on arrays of bit patterns.
#include <stddef.h>

#include "../neural_inventory_control_amd/csrc/nic_bf16.h"

extern "C" void nic_test_f32_to_bf16(const float* in, uint16_t* out, size_t n) {
    for (size_t i = 0; i < n; ++i) out[i] = nic_f32_to_bf16_bits(in[i]);
}
