// The launch plan of the weight-gradient GEMMs (linear_mfma.hip, linear_bf16.hip): which kernel runs for a shape, how the slab
// slots factor into scenario splits x period groups, the chunk size, the flush interval and how the horizon is cut into
// launches.  Plain C++ on stack values - no HIP, no allocation, no environment (tests/test_wgrad_plan_host.py compiles it with the
// host compiler alone).  A new weight-gradient route is added HERE: a WgradTile, its classifier, its line in wgrad_plan.
#pragma once
#include <stdint.h>
#include "../../include/nic_rollout.h"   // NIC_THIN_MAX_ROWS

namespace nic {


constexpr int kWgradBK = 32;   // k depth (scenarios) of one LDS tile: chunks are multiples of it
inline int wgrad_ceil_div(int a, int b) { return (a + b - 1) / b; }
inline int wgrad_clamp(int v, int lo, int hi) { return v > hi ? (hi > lo ? hi : lo) : (v > lo ? v : lo); }   // max(lo, min(v, hi))

// ---- shape classifiers and tile tables ---------------------------------------------------------------------------------------
// Every kernel of the weight gradient; a shape's tile is a function of (N, K) only, so that slot counts and launches agree
enum WgradTile {
    WG_SMALL_1, WG_SMALL_2, WG_SMALL_3, WG_SMALL_4,                  // wgrad_small_kernel<KC>: N <= 32, K <= 32 KC
    WG_DMA_TALL, WG_DMA_HALF, WG_DMA_MID, WG_DMA_WIDE5, WG_DMA_WIDE6, WG_DMA_WIDE7, WG_DMA_BIG,   // gemm_wgrad_dma_kernel
    WG_STAGED_128x128, WG_STAGED_128x64, WG_STAGED_64x128, WG_STAGED_32x256,                      // gemm_wgrad_kernel
};
// register-staged tile (rows x columns of the output, the bias column K included) and its output tiles per scenario chunk
inline WgradTile wgrad_tile(int N, int K) {
    if (N > 64) return K + 1 > 64 ? WG_STAGED_128x128 : WG_STAGED_128x64;
    return N > 32 ? WG_STAGED_64x128 : WG_STAGED_32x256;
}
inline int wgrad_staged_tiles(int N, int K) {
    constexpr int dims[4][2] = {{128, 128}, {128, 64}, {64, 128}, {32, 256}};   // in WgradTile order
    const int* d = dims[wgrad_tile(N, K) - WG_STAGED_128x128];
    return wgrad_ceil_div(N, d[0]) * wgrad_ceil_div(K + 1, d[1]);
}

// big layers: 256 x 256 LDS-DMA tiles, one workgroup per CU
inline bool wgrad_big(int N, int K) { return N >= 192 && K >= 129; }
// N >= 192 output rows over 65..128 input rows (the shipped many-warehouse setting's first layer: 512 x 66): 256 x 128 tiles on
// the LDS-DMA pipeline (round 4; the register-staged 128 x 128 kernel ran that layer's all-period gradient at 0.02 of peak)
inline bool wgrad_half(int N, int K) { return N >= 192 && K > 64 && K <= 128; }
// tall, narrow layers (the first layer: 512 x 51): ONE 512 x 64 output tile per scenario chunk, so dZ is read exactly once
// (the 128 x 64 register-staged tiles read it 1.3 x) by the LDS-DMA pipeline; HBM-bound
inline bool wgrad_tall(int N, int K) { return N >= 384 && K <= 64; }
// K in (256, 448] (cfg5's first layer: 393 input rows, 295 of them live): ONE 320 / 384 / 448-column tile covers it (88 % of the
// tile's columns used at K = 393) where two 256-column tiles compute 512 (77 %); 128 x 448 keeps the 112 accumulator registers
// of the 7-tile wx kernel
inline bool wgrad_wide(int N, int K) { return wgrad_big(N, K) && K > 256 && K <= 448 && N % 128 == 0; }
inline int wgrad_wide_nt(int K) { return (K + 63) / 64; }   // 5, 6 or 7 column tiles of 32 per wave column: 320 / 384 / 448 columns
// 96 <= N <= 128 output rows over a wide input (cfg5's compacted logits layer, 98 x 512): 128 x 256 tiles on the LDS-DMA pipeline
// (the register-staged 128 x 128 kernel reaches 0.37 of peak there)
inline bool wgrad_mid(int N, int K) { return N >= 96 && N <= 128 && K >= 192; }
inline bool wgrad_dma_shape(int N, int K) { return wgrad_big(N, K) || wgrad_tall(N, K) || wgrad_mid(N, K) || wgrad_half(N, K); }
// output tiles of one scenario chunk under the LDS-DMA kernel wgrad_dma_tile picks (what the split counts divide 256 by)
inline int wgrad_dma_tiles(int N, int K) {
    if (wgrad_tall(N, K)) return (N + 511) / 512;
    if (wgrad_half(N, K)) return (N + 255) / 256;
    if (wgrad_mid(N, K)) return (K + 255) / 256;
    if (wgrad_wide(N, K)) return (N + 127) / 128;
    return ((N + 127) / 128) * ((K + 255) / 256);
}
// the LDS-DMA weight-gradient kernel for a shape (wgrad_dma_shape)
inline WgradTile wgrad_dma_tile(int N, int K) {
    if (wgrad_tall(N, K)) return WG_DMA_TALL;
    if (wgrad_half(N, K)) return WG_DMA_HALF;
    if (wgrad_mid(N, K)) return WG_DMA_MID;
    if (wgrad_wide(N, K)) return wgrad_wide_nt(K) == 5 ? WG_DMA_WIDE5 : (wgrad_wide_nt(K) == 6 ? WG_DMA_WIDE6 : WG_DMA_WIDE7);
    // big layers: 128 x 256 tiles (round 4; wave tile 64 x 64 = 64 accumulator registers, no scratch).  Measured against round 3's
    // 256 x 256 tile (128 accumulators, 516 B of scratch) on 512 x 512 x 16,384 x T=50: 133.3-133.9 against 131.8 TFLOP/s
    // (profiles/r04_gemm_stagger_and_wgrad_tile_probe.json)
    return WG_DMA_BIG;
}
// thin output (N <= 32 rows), up to 128 input features: one wave per split, 1..4 accumulators
inline WgradTile wgrad_small_tile(int K) { return K <= 32 ? WG_SMALL_1 : (K <= 64 ? WG_SMALL_2 : (K <= 96 ? WG_SMALL_3 : WG_SMALL_4)); }
// ---- slab slots --------------------------------------------------------------------------------------------------------------
// slot = period group * scen_splits + scenario split; a scenario split contracts `chunk` scenarios (a multiple of 32), a group
// `periods_per_group` periods
struct WgradSlots { int scen_splits, groups, chunk, periods_per_group; };
inline int wgrad_chunk(int n_scenarios, int scen_splits) { return wgrad_ceil_div(wgrad_ceil_div(n_scenarios, scen_splits), kWgradBK) * kWgradBK; }
// every slot a scenario split of all the periods
inline WgradSlots scenario_slots(int n_slots, int n_scenarios, int n_periods) { return {n_slots, 1, wgrad_chunk(n_scenarios, n_slots), n_periods}; }
// Slab slots of the all-period contraction as (scenario splits x period groups): scenario chunks go down to 128 scenarios (4 k
// tiles per period), what is still missing to fill the chip comes from splitting the horizon.
inline WgradSlots period_factors(int n_slots, int n_scenarios, int n_periods) {
    const int ss = wgrad_clamp(n_slots, 1, n_scenarios / 128), g = wgrad_clamp(n_slots / ss, 1, n_periods);
    return {ss, g, wgrad_chunk(n_scenarios, ss), wgrad_ceil_div(n_periods, g)};
}
// An fp32 sum of 10^5 terms in one register drifts to ~5e-5 relative (see WgParams::flush_periods): no accumulator sums more
// than ~8k terms (chunk x periods) before it is added to the slab.
constexpr int kWgradMaxTerms = 8192;
inline int wgrad_flush_periods(int chunk) { return wgrad_clamp(kWgradMaxTerms / chunk, 1, kWgradMaxTerms); }
// ---- recommended slot counts (nic_wgrad_num_splits, nic_wgrad_periods_num_splits) -------------------------------------------------
inline int wgrad_recommended_slots(int N, int K, int n_scenarios, int cus) {
    if (N <= 0 || K <= 0 || n_scenarios <= 0) return 0;
    // (N <= 32, K = 64 / 96 / 128 counts as a thin layer here though wgrad_plan runs wgrad_small_kernel: kept ON PURPOSE, a tuning matter)
    if (N <= 32 && (K <= 32 || (K <= 128 && K % 32 != 0))) {  // wgrad_small_kernel: one split per wave, >= 2048 columns each
        return (wgrad_clamp((int)(((int64_t)n_scenarios + 2047) / 2048), 1, 1024) + 3) / 4 * 4;  // at most one wave per SIMD
    }
    if (N <= NIC_THIN_MAX_ROWS && K % 32 == 0) {  // nic_linear_bwd_thin: one wave per (split, 32-row chunk), 2 waves per SIMD
        return wgrad_clamp(2048 / (K / 32), 1, (n_scenarios + 63) / 64);  // at least one 64-scenario block per split
    }
    // LDS-DMA tiles: one workgroup per CU, one round; register-staged: ~4 workgroups per CU in total
    const int fill = wgrad_dma_shape(N, K) ? wgrad_ceil_div(cus, wgrad_dma_tiles(N, K)) : wgrad_ceil_div(4 * cus, wgrad_staged_tiles(N, K));
    return wgrad_clamp(fill, 1, (n_scenarios + 255) / 256);  // at least 256 scenarios (8 k-tiles) per split
}
inline int wgrad_periods_recommended_slots(int N, int K, int n_scenarios, int n_periods, int cus) {
    if (N <= 0 || K <= 0 || n_scenarios <= 0 || n_periods <= 0) return 0;
    if (N <= 32 && K <= 32) return wgrad_recommended_slots(N, K, n_scenarios, cus);   // wgrad_small_kernel: one launch per period
    if (!wgrad_dma_shape(N, K) || n_scenarios % kWgradBK != 0) {
        // register-staged kernels (ragged scenario counts, narrow layers: the real-data batches of 72-288 products x 95 weeks):
        // the same (period group x scenario split) slots - ONE launch instead of a serial walk over the horizon by 1-4 workgroups
        const WgradSlots s = period_factors(wgrad_ceil_div(4 * cus, wgrad_staged_tiles(N, K)), n_scenarios, n_periods);
        const int base = wgrad_recommended_slots(N, K, n_scenarios, cus);
        return s.scen_splits * s.groups > base ? s.scen_splits * s.groups : base;
    }
    const WgradSlots s = period_factors(wgrad_ceil_div(cus, wgrad_dma_tiles(N, K)), n_scenarios, n_periods);   // one workgroup per CU, one round
    return s.scen_splits * s.groups;
}
// ---- operand eligibility -----------------------------------------------------------------------------------------------------
// `buffer`: the buffer-load paths (wgrad_small_kernel, the FAST form of gemm_wgrad_kernel) - 16-byte aligned dY and X, row stride a
// multiple of 4 floats, both operands below 2^28 floats.  `dma`: the LDS-DMA kernel, which also writes the slab as float4 rows -
// 16-byte aligned slab, slab row stride a multiple of 4 (its third condition, n_scenarios % 32 == 0, is checked by wgrad_plan).
struct WgradOperands { bool buffer, dma; };
// dyx_address / slab_address: byte addresses (dY and X OR-ed together; the slab) - only the low 4 bits count
inline WgradOperands wgrad_operands(uint64_t dyx_address, uint64_t slab_address, int64_t ldb, int64_t lds, int N, int K) {
    const bool buffer = ldb % 4 == 0 && (dyx_address & 15) == 0 && (int64_t)N * ldb < (1ll << 28) && (int64_t)K * ldb < (1ll << 28);
    return {buffer, buffer && lds % 4 == 0 && (slab_address & 15) == 0};
}

// ---- the plan ----------------------------------------------------------------------------------------------------------------
enum WgradEntry { WG_ONE_PERIOD /* nic_linear_wgrad */, WG_ALL_PERIODS /* nic_linear_wgrad_periods */ };
// how the horizon is cut into launches of `launch_periods` consecutive periods (the last launch: the rest).  WG_PER_PERIOD
// launches are nic_linear_wgrad calls: period strides 0, errors under that name.
enum WgradCut { WG_ONE_LAUNCH, WG_PER_PERIOD, WG_PER_GROUP };
struct WgradPlan {
    WgradTile tile, tile_single;   // kernel of a launch of two or more periods / of exactly one (wgrad_small_kernel contracts one)
    int slots;                     // slab slots the launches address (<= the slots given; the others stay untouched)
    int chunk, scen_splits, periods_per_group, flush_periods;   // as WgParams: scen_splits = periods_per_group = 0 when every slot
                                   // is a scenario split of all the launch's periods; flush_periods = 0: one slab update, at the end
    WgradCut cut;
    int launch_periods;
};
struct WgradLaunch { int first_period, n_periods; WgradTile tile; };
// the launches of a plan: first_period = 0, then first_period + n_periods, while n_periods > 0
inline WgradLaunch wgrad_launch(const WgradPlan& p, int n_periods, int first_period) {
    const int n = n_periods - first_period < p.launch_periods ? n_periods - first_period : p.launch_periods;
    return {first_period, n, n == 1 ? p.tile_single : p.tile};
}
// force_staged: tuning builds only (NIC_GEMM_VARIANT=2, the register-staged kernels on LDS-DMA shapes)
inline WgradPlan wgrad_plan(WgradEntry entry, int N, int K, int n_scenarios, int n_periods, int n_splits, WgradOperands ops,
                            bool force_staged = false) {
    const bool dma = wgrad_dma_shape(N, K) && ops.dma && n_scenarios % kWgradBK == 0 && !force_staged;
    const WgradTile many = dma ? wgrad_dma_tile(N, K) : wgrad_tile(N, K);
    const WgradTile single = N <= 32 && K <= 128 && ops.buffer ? wgrad_small_tile(K) : many;
    const int chunk = wgrad_chunk(n_scenarios, n_splits);   // every slot a scenario split
    // one period per launch: nic_linear_wgrad itself, and off the LDS-DMA path a horizon of one period or a tiny layer
    if (entry == WG_ONE_PERIOD || (!dma && (n_periods == 1 || (N <= 32 && K <= 32))))
        return {single, single, n_splits, chunk, 0, 0, 0, entry == WG_ONE_PERIOD ? WG_ONE_LAUNCH : WG_PER_PERIOD, 1};
    const WgradSlots s = period_factors(n_splits, n_scenarios, n_periods);
    // LDS-DMA: ONE launch over (period group, scenario split) slots, partial sums flushed to the slab every ~8k terms
    if (dma)
        return {many, many, s.scen_splits * s.groups, s.chunk, s.scen_splits, s.periods_per_group, wgrad_flush_periods(s.chunk),
                WG_ONE_LAUNCH, n_periods};
    // register-staged kernels (they loop over the periods themselves, without flushing).  With enough slab slots: ONE launch,
    // slot = (period group, scenario split), as long as no accumulator sums more than ~8k terms (chunk x periods per group)
    if (s.groups > 1 && (int64_t)s.chunk * s.periods_per_group <= kWgradMaxTerms)
        return {many, many, s.scen_splits * s.groups, s.chunk, s.scen_splits, s.periods_per_group, 0, WG_ONE_LAUNCH, n_periods};
    // otherwise: a launch per group of periods, so that no accumulator sums more than ~8k terms before it is added to the slab
    return {many, single, n_splits, chunk, 0, 0, 0, WG_PER_GROUP, wgrad_clamp(kWgradMaxTerms / wgrad_ceil_div(n_scenarios, n_splits), 1, kWgradMaxTerms)};
}

}  // namespace nic
