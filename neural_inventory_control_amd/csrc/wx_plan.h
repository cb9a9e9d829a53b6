// The launch plan of the forward / input-gradient ("wx") GEMMs (linear_mfma.hip, linear_bf16.hip): which kernel instantiation
// runs for a shape, over which grid, and under which name nic_last_kernel() reports it.  Plain C++ on stack values - no HIP, no
// allocation, no environment; the compute-unit count is an argument (tests/test_wx_plan_host.py compiles it with the host compiler
// alone).  A new wx kernel is added HERE: a WxKernel, its line in kWxGeometry, its condition in wx_plan - and its launcher in
// kWxLaunch (linear_mfma.hip).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

namespace nic {

// ---- the kernels -------------------------------------------------------------------------------------------------------------
// Every instantiation the dispatch can launch.  From WX_PRODUCT_END on: tuning builds only (-DNIC_TUNING_BUILD), reached through a
// WxForce and never through the pickers.
enum WxKernel {
    WX_STREAM_1x2, WX_STREAM_1x4,                          // gemm_wx_stream_kernel<NT,KS>
    WX_DMA_128x128, WX_DMA_64x128, WX_DMA_32x128,          // gemm_wx_dma_kernel<WM,WN,MT,NT>
    WX_STAGED_128x128, WX_STAGED_64x128, WX_STAGED_32x256,  // gemm_wx_kernel<WM,WN,MT,NT>
    WX_PRODUCT_END,
    WX_STREAM_1x1 = WX_PRODUCT_END, WX_STREAM_2x1, WX_STREAM_2x2, WX_STREAM_2x4, WX_DMA_256x256,
    WX_KERNEL_END
};
enum WxFamily { WX_STREAM, WX_DMA, WX_STAGED };
// targs: the template arguments in front of EPI (streamed: NT, KS; the others: WM, WN, MT, NT); bm x bn: the output block of one
// workgroup; threads: its size
struct WxGeometry { WxFamily family; int targs[4]; int bm, bn, threads; };
constexpr WxGeometry kWxGeometry[WX_KERNEL_END] = {
    {WX_STREAM, {1, 2}, 32, 32, 128},         {WX_STREAM, {1, 4}, 32, 32, 256},
    {WX_DMA, {2, 4, 2, 1}, 128, 128, 512},    {WX_DMA, {2, 4, 1, 1}, 64, 128, 512},    {WX_DMA, {1, 4, 1, 1}, 32, 128, 256},
    {WX_STAGED, {2, 2, 2, 2}, 128, 128, 256}, {WX_STAGED, {1, 4, 2, 1}, 64, 128, 256}, {WX_STAGED, {1, 4, 1, 2}, 32, 256, 256},
    {WX_STREAM, {1, 1}, 32, 32, 64},          {WX_STREAM, {2, 1}, 32, 64, 64},         {WX_STREAM, {2, 2}, 32, 64, 128},
    {WX_STREAM, {2, 4}, 32, 64, 256},         {WX_DMA, {2, 4, 4, 2}, 256, 256, 512},
};
inline int wx_grid(WxKernel k, int M, int ncols) {
    return ((M + kWxGeometry[k].bm - 1) / kWxGeometry[k].bm) * ((ncols + kWxGeometry[k].bn - 1) / kWxGeometry[k].bn);
}
// the name nic_last_kernel() reports; epi: "EPI_BIAS_ACT" (forward) or "EPI_DGRAD"
inline void wx_kernel_name(char* out, size_t size, WxKernel k, const char* epi) {
    const int* a = kWxGeometry[k].targs;
    if (kWxGeometry[k].family == WX_STREAM) snprintf(out, size, "gemm_wx_stream_kernel<%d,%d,%s>", a[0], a[1], epi);
    else snprintf(out, size, kWxGeometry[k].family == WX_DMA ? "gemm_wx_dma_kernel<%d,%d,%d,%d,%s>" : "gemm_wx_kernel<%d,%d,%d,%d,%s>",
                  a[0], a[1], a[2], a[3], epi);
}

// ---- operand eligibility -----------------------------------------------------------------------------------------------------
// fast (buffer-load) path: 16-byte aligned operands, row strides multiples of 4 floats, buffers below 2^28 floats.
// ab_address: the byte addresses of A and B OR-ed together - only the low 4 bits count
inline bool wx_operands(uint64_t ab_address, int64_t lda, int64_t ldb, int M, int K) {
    return lda % 4 == 0 && ldb % 4 == 0 && (ab_address & 15) == 0 && (int64_t)M * lda < (1ll << 28) && (int64_t)K * ldb < (1ll << 28);
}

// ---- the pickers -------------------------------------------------------------------------------------------------------------
// Tile shape of the LDS-DMA wx kernel.  Round 4 measured seventeen tilings from 1,024 to 65,536 scenarios
// (tools/gemm_tile_probe.py, profiles/r04_gemm_tile_probe*.json) and what decides is NOT bytes of LDS traffic per flop but how
// many workgroups a CU holds at once: a lone 256 x 256 workgroup (128 KB of LDS, one per CU) spends ~0.5-1.2 us of every k tile
// in the copy's round trip + the barrier with nothing else to issue, while two co-resident 128 x 128 workgroups of 8 waves
// (64 KB each, 65-90 VGPRs) cover each other's stalls: 512 x 512 x 65,536 dgrad 278 -> 262 us (0.786 -> 0.833 of the FP32 MFMA
// peak), forward 267 = 267; at 8,192 scenarios (cfg3's shard on 8 GPUs) 73 -> 38-40 us, at 1,024 (the reference's shipped
// batch) 70 -> 14 us.  Round 3's picker counted whole rounds of 256 CUs only, so every launch of fewer than 256 tiles "cost one
// round" whatever the tile and ran as 16-128 big workgroups.  Three tilings remain:
//   128 x 128, 8 waves (wave tile 64 x 32), 2 per CU   launches that fill both slots of every CU (>= 512 tiles)
//    64 x 128, 8 waves (wave tile 32 x 32), 3 per CU   smaller launches with >= 33 output rows
//    32 x 128, 4 waves (wave tile 32 x 32), 4 per CU   thin outputs (17 logits rows) and ragged heights (393 rows: 13 row
//                                                      blocks of 32 instead of 4 of 128 - measured 229 us against 252 for
//                                                      round 3's 448-row tile)
// chosen by rows computed per row of the matrix (padding to the block height) x the measured relative cost of the tiling.
// The 256 x 256 tiling only exists in tuning builds (A/B reference of the probes).
inline WxKernel pick_wx_tile(int M, int ncols, int cus) {
    auto padded = [&](int bm) { return (double)((M + bm - 1) / bm * bm) / M; };
    const int64_t tiles128 = (int64_t)((M + 127) / 128) * ((ncols + 127) / 128);
    double c128 = padded(128), c64 = padded(64) * 1.02, c32 = padded(32) * 1.06;   // (512 x 512 x 65,536: 262 / 265 / 281 us)
    if (tiles128 < 2 * cus) {   // fewer than two workgroups per CU: smaller tiles put more wavefronts on a CU
        c128 = 1e30;
        c64 = padded(64);
        c32 = padded(32) * 1.02;
    }
    if (c128 <= c64 && c128 <= c32) return WX_DMA_128x128;
    return c64 <= c32 ? WX_DMA_64x128 : WX_DMA_32x128;
}

// Streamed form (gemm_wx_stream_kernel) for launches of at most 1,024 output tiles of 32 x 32: NT = 1 (every tile its own
// wavefront), KS = wavefronts that split the contraction, so that the launch has ~2,048 wavefronts where K allows.
// Returns 0 (LDS-DMA kernels) or KS.  Measured (tools/gemm_tile_probe.py --stream, profiles/r04_gemm_stream_probe.json; us per
// launch, LDS-DMA -> streamed): 512 x 512 x 1,024 scenarios 21.7 -> 10.5, x 2,048 22.8 -> 15.7, x 4,096 25.0 -> 29.4 (not taken);
// logits 17 x 512 13.2 -> 7.5 up to 8,192 scenarios, 14.5 -> 9.3 at 16,384; first-layer input gradient 51 x 512 20.6 -> 7.6.
// (KS is 2 or 4, never 1: with tiles <= 4 cus and K >= 128 the first pass of the loop always succeeds)
inline int pick_wx_stream(int M, int K, int ncols, int cus) {
    const int64_t tiles = (int64_t)((M + 31) / 32) * ((ncols + 31) / 32);
    if (tiles > 4 * cus || K < 128) return 0;   // (a short contraction is 2-4 k tiles of the LDS pipeline: nothing to gain, measured)
    int ks = 1;
    while (ks < 4 && tiles * ks * 2 <= 8 * cus && K >= 64 * ks * 2) ks *= 2;
    return ks;
}

// ---- the plan ----------------------------------------------------------------------------------------------------------------
// What a tuning build forces on operands of the fast path (-1: nothing, the pickers decide).
//   stream: NIC_WX_STREAM - 10 * NT + KS = that streamed instantiation for every launch, any other value = never streamed
//   tile:   NIC_WX_TILE / tune bit 128 - 0..3 = LDS-DMA 128 x 128, 64 x 128, 32 x 128, 256 x 256 for every launch not streamed
struct WxForce { int stream = -1, tile = -1; };
struct WxPlan { WxKernel kernel; int grid; };
inline WxPlan wx_plan(int M, int K, int ncols, bool operands_ok, int cus, WxForce force = {}) {
    WxKernel k;
    if (!operands_ok) {   // unaligned operands: guarded register-staged kernels
        k = M > 64 ? WX_STAGED_128x128 : (M > 32 ? WX_STAGED_64x128 : WX_STAGED_32x256);
    } else {
        constexpr WxKernel tiles[4] = {WX_DMA_128x128, WX_DMA_64x128, WX_DMA_32x128, WX_DMA_256x256};
        const int nt_ks = force.stream >= 0 ? force.stream : 10 + pick_wx_stream(M, K, ncols, cus);
        switch (nt_ks) {
            case 11: k = WX_STREAM_1x1; break;
            case 12: k = WX_STREAM_1x2; break;
            case 14: k = WX_STREAM_1x4; break;
            case 21: k = WX_STREAM_2x1; break;
            case 22: k = WX_STREAM_2x2; break;
            case 24: k = WX_STREAM_2x4; break;
            default: k = force.tile >= 0 && force.tile < 4 ? tiles[force.tile] : pick_wx_tile(M, ncols, cus);   // LDS-DMA kernels
        }
    }
    return {k, wx_grid(k, M, ncols)};
}

// the bf16 wx kernels (linear_bf16.hip, bf16_wx_kernel<MT,NT>): 128 x 128 tiles (wave tile 64 x 64) for big launches, 64 x 64
// tiles - four times the workgroups - below two 128 x 128 tiles per CU
struct Bf16WxTile { int mt_nt; int64_t grid; };   // bf16_wx_kernel<mt_nt, mt_nt, EPI>
inline Bf16WxTile bf16_wx_tile(int M, int ncols, int cus) {
    const int64_t tiles128 = (int64_t)((M + 127) / 128) * ((ncols + 127) / 128);
    if (tiles128 >= 2 * cus) return {2, tiles128};
    return {1, (int64_t)((M + 63) / 64) * ((ncols + 63) / 64)};
}

}  // namespace nic
