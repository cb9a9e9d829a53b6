// Host build of the weight-gradient launch plan (csrc/wgrad_plan.h) for tests/test_wgrad_plan_host.py: compiled with the host
// compiler into a small shared library and called through ctypes on arrays of cases.
#include <stddef.h>

#include "../neural_inventory_control_amd/csrc/wgrad_plan.h"

extern "C" {

// in: n x {N, K, B, T}; out: n x {nic_wgrad_num_splits, nic_wgrad_periods_num_splits} at `cus` compute units
void nic_test_wgrad_slots(const int32_t* in, int32_t* out, size_t n, int cus) {
    for (size_t i = 0; i < n; ++i) {
        const int32_t* c = in + 4 * i;
        out[2 * i] = nic::wgrad_recommended_slots(c[0], c[1], c[2], cus);
        out[2 * i + 1] = nic::wgrad_periods_recommended_slots(c[0], c[1], c[2], c[3], cus);
    }
}

// in: n x {entry (0 = one period, 1 = all periods), N, K, B, T, slots given, operands buffer-eligible, operands DMA-eligible}
// out: n x {the 9 plan fields; number of launches; periods covered (sum over the launches, each starting where the last ended);
//           launches of one period that run wgrad_small_kernel; launches of more than one period that do}
void nic_test_wgrad_plans(const int32_t* in, int32_t* out, size_t n) {
    for (size_t i = 0; i < n; ++i) {
        const int32_t* c = in + 8 * i;
        const nic::WgradPlan p = nic::wgrad_plan(c[0] ? nic::WG_ALL_PERIODS : nic::WG_ONE_PERIOD, c[1], c[2], c[3], c[4], c[5],
                                                 nic::WgradOperands{c[6] != 0, c[7] != 0});
        int launches = 0, covered = 0, small_single = 0, small_many = 0, next = 0;
        for (nic::WgradLaunch l = nic::wgrad_launch(p, c[4], 0); l.n_periods > 0; l = nic::wgrad_launch(p, c[4], next)) {
            if (l.first_period != next) covered = -1000000;   // a gap or an overlap
            next = l.first_period + l.n_periods;
            ++launches;
            covered += l.n_periods;
            if (l.tile <= nic::WG_SMALL_4) ++(l.n_periods == 1 ? small_single : small_many);
            if (l.tile != (l.n_periods == 1 ? p.tile_single : p.tile)) covered = -1000000;
        }
        const int32_t row[13] = {p.tile, p.tile_single, p.slots, p.chunk, p.scen_splits, p.periods_per_group, p.flush_periods, p.cut,
                                 p.launch_periods, launches, covered, small_single, small_many};
        for (int j = 0; j < 13; ++j) out[13 * i + j] = row[j];
    }
}

const char* nic_test_wgrad_tile_name(int tile) {
    static const char* const names[] = {"small<1>", "small<2>", "small<3>", "small<4>", "dma_tall", "dma_half", "dma_mid",
                                        "dma_wide5", "dma_wide6", "dma_wide7", "dma_big", "staged_128x128", "staged_128x64",
                                        "staged_64x128", "staged_32x256"};
    return tile >= nic::WG_SMALL_1 && tile <= nic::WG_STAGED_32x256 ? names[tile] : "?";
}

// the operand-eligibility helper: bit 0 = buffer-load paths, bit 1 = LDS-DMA kernel
int nic_test_wgrad_operands(uint64_t dyx_address_bits, uint64_t slab_address_bits, int64_t ldb, int64_t lds, int N, int K) {
    const nic::WgradOperands o = nic::wgrad_operands(dyx_address_bits, slab_address_bits, ldb, lds, N, K);
    return (o.buffer ? 1 : 0) | (o.dma ? 2 : 0);
}
}
