// Opt-in bf16 matrix-core GEMMs for the wide hidden-to-hidden policy layers (FusedRollout.gemm_precision = "bf16").  OUTSIDE the
// 1e-5 parity contract of the FP32 kernels (linear_mfma.hip): operands are rounded to bf16 (round to nearest even) on the way
// into v_mfma_f32_32x32x16_bf16; products are exact in FP32, accumulation, bias, ELU and ELU' stay FP32.
//
// Formulation (feature-major activations, as linear_mfma.hip):
//     forward   Y[n][b]  = act( sum_k bf16(W[n][k])  bf16(X[k][b])  + bias[n] )     A = W   bf16 [N][ldw] (engine copy)
//     dgrad     dX[k][b] = ( sum_n bf16(Wt[k][n]) bf16(dY[n][b]) ) * act'(H[k][b])   A = W^T bf16 [K][ldwt] (engine copy)
//     wgrad     slab[n][k] += sum_b bf16(dY[n][b]) bf16(X[k][b]);  slab[n][K] += sum_b dY[n][b]   (bias column: FP32 sum)
// Operand lane map of v_mfma_f32_32x32x16_bf16 (cdna_hip_programming.md §3): lane l (r = l & 31, h = l >> 5) holds
// A[row r][k = 8h + j] and B[k = 8h + j][col r], j = 0..7 - eight CONSECUTIVE k of one row / column, one ds_read_b128 from a
// k-contiguous LDS image.  C/D: col = l & 31, row = (reg & 3) + 8 (reg >> 2) + 4h.
//
// Staging (register-staged, double-buffered LDS, one barrier per 32-deep k tile):
//   A of the wx kernel: bf16 rows [m][k], k-contiguous in memory: 16-byte loads straight into the [m][k] LDS image.
//   B of the wx kernel (X or dY, [K][ldb], k-STRIDED): each thread loads KPT rows x 4 consecutive columns as float4s (coalesced
//     128-byte+ runs per row), converts in registers and writes, per column, its KPT consecutive k as one 8- or 4-byte store
//     into a TRANSPOSED [b][k] bf16 image: the fragment read is then the same ds_read_b128 as A's.
//   Both operands of the wgrad kernel are [row][b] with the contraction (scenario) contiguous: float4 loads, convert, [row][b]
//     images.
//   LDS rows are 40 bf16 (32 k + 8 pad = 80 bytes): the 16 lanes of a ds_read_b128 group read 16 consecutive rows = 16 distinct
//     bank quads (80 B = 20 dwords; 20 r mod 64 takes 16 distinct multiples of 4 for r = 0..15); the transposing writes
//     (lanes: 8 or 16 k groups x 2-4 column groups per half wave) are conflict-free as well.
// Roofline: with FP32 activations in HBM the layers are bandwidth-bound, not MFMA-bound - 512 x 512 x 65,536 scenarios streams
// X (134 MB) in and Y (134 MB) out per forward (+ Hprev 134 MB per dgrad) against 34 GFLOP, 1 % of the bf16 MFMA peak's time.
// No atomics (every slab element has one owner workgroup: results are deterministic run to run); no inline asm.
#include "nic_common.h"
#include "nic_bf16.h"
#include "wgrad_plan.h"
#include "wx_plan.h"

namespace {

using bf16x8 = __attribute__((ext_vector_type(8))) __bf16;
using f32x16 = __attribute__((ext_vector_type(16))) float;

constexpr int BK = 32;        // k depth of one LDS tile
constexpr int LROW = 40;      // LDS row in bf16 elements (32 + 8 pad, see above)
constexpr int kThreads = 256; // 4 waves, 2 x 2 over the output tile

enum { EPI_BIAS_ACT = 0, EPI_DGRAD = 1 };

// The FP32 kernels' ELU and ELU' (linear_mfma.hip): the same epilogue arithmetic in both precisions.
__device__ __forceinline__ float elu_f(float x) {
    const float xn = fminf(x, 0.f);
    const float series =
        xn * fmaf(xn, fmaf(xn, fmaf(xn, fmaf(xn, fmaf(xn, 1.f / 720.f, 1.f / 120.f), 1.f / 24.f), 1.f / 6.f), 0.5f), 1.f);
    const float viaexp = __expf(xn) - 1.f;
    const float neg = xn > -0.35f ? series : viaexp;
    return x > 0.f ? x : neg;
}
__device__ __forceinline__ float elu_grad_from_out(float y) { return y > 0.f ? 1.f : y + 1.f; }

// XCD-aware tile order (linear_mfma.hip): every XCD gets a contiguous range of logical tiles, so the row tiles that share a
// scenario panel run on one XCD's L2.  Bijective for any grid size.
__device__ __forceinline__ int xcd_swizzle(int bid, int nwg) {
    const int q = nwg >> 3, r = nwg & 7, xcd = bid & 7, idx = bid >> 3;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
}

__device__ __forceinline__ uint2 cvt4(float4 v) { return make_uint2(nic_pack_bf16x2(v.x, v.y), nic_pack_bf16x2(v.z, v.w)); }

// ---------------------------------------------------------------------------------------------------------------
// wx kernel: C[M][ncols] = epilogue( A[M][K] (bf16) * bf16(Bm[K][ldb]) ).  K % 32 == 0; rows >= M and columns >= ncols are
// zero-filled on load and not written.
// ---------------------------------------------------------------------------------------------------------------
struct WxParams {
    const __bf16* A;     // [M][lda] bf16, 16-byte aligned rows
    int64_t lda;
    const float* Bm;     // [K][ldb]
    float* C;            // [M][ldb]
    const float* bias;   // [M] or null (EPI_BIAS_ACT)
    const float* Hprev;  // [M][ldb] or null (EPI_DGRAD)
    int M, K, ncols;     // ncols: multiple of 4, <= ldb
    int64_t ldb;
    int act, accumulate;
};

template <int MT, int NT, int EPI>
__global__ __launch_bounds__(kThreads) void bf16_wx_kernel(WxParams p) {
    constexpr int BM = 2 * MT * 32, BN = 2 * NT * 32;
    constexpr int A_CH = BM * 4 / kThreads;          // 16-byte A chunks per thread per tile
    constexpr int CG = BN / 4, KG = kThreads / CG;   // B tile: column groups of 4 x k groups
    constexpr int KPT = BK / KG;                     // k rows per thread (4 or 2)
    static_assert(KPT == 2 || KPT == 4, "B tile staging");
    __shared__ __attribute__((aligned(16))) __bf16 sA[2][BM * LROW];
    __shared__ __attribute__((aligned(16))) __bf16 sB[2][BN * LROW];

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, wm = wave >> 1, wn = wave & 1;
    const int li = lane & 31, h = lane >> 5;
    const int tiles_m = (p.M + BM - 1) / BM;
    const int tile = xcd_swizzle(blockIdx.x, gridDim.x);
    const int m0 = (tile % tiles_m) * BM, c0 = (tile / tiles_m) * BN;
    const int kg = t % KG, cg = t / KG, bcol = c0 + cg * 4;
    const bool bcol_ok = bcol < p.ncols;

    uint4 ra[A_CH];
    float4 rb[KPT];
    auto load = [&](int k0) {
#pragma unroll
        for (int i = 0; i < A_CH; ++i) {
            const int idx = t + kThreads * i, r = idx >> 2, q = idx & 3, row = m0 + r;
            ra[i] = row < p.M ? *reinterpret_cast<const uint4*>(p.A + (int64_t)row * p.lda + k0 + q * 8) : make_uint4(0, 0, 0, 0);
        }
#pragma unroll
        for (int i = 0; i < KPT; ++i) {
            const int k = k0 + kg * KPT + i;
            rb[i] = bcol_ok ? *reinterpret_cast<const float4*>(p.Bm + (int64_t)k * p.ldb + bcol) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    };
    auto store = [&](int buf) {
#pragma unroll
        for (int i = 0; i < A_CH; ++i) {
            const int idx = t + kThreads * i, r = idx >> 2, q = idx & 3;
            *reinterpret_cast<uint4*>(&sA[buf][r * LROW + q * 8]) = ra[i];
        }
        // transpose: column cg * 4 + j of the tile gets this thread's KPT consecutive k
        __bf16* col0 = &sB[buf][(cg * 4) * LROW + kg * KPT];
        if constexpr (KPT == 4) {
            *reinterpret_cast<uint2*>(col0 + 0 * LROW) =
                make_uint2(nic_pack_bf16x2(rb[0].x, rb[1].x), nic_pack_bf16x2(rb[2].x, rb[3].x));
            *reinterpret_cast<uint2*>(col0 + 1 * LROW) =
                make_uint2(nic_pack_bf16x2(rb[0].y, rb[1].y), nic_pack_bf16x2(rb[2].y, rb[3].y));
            *reinterpret_cast<uint2*>(col0 + 2 * LROW) =
                make_uint2(nic_pack_bf16x2(rb[0].z, rb[1].z), nic_pack_bf16x2(rb[2].z, rb[3].z));
            *reinterpret_cast<uint2*>(col0 + 3 * LROW) =
                make_uint2(nic_pack_bf16x2(rb[0].w, rb[1].w), nic_pack_bf16x2(rb[2].w, rb[3].w));
        } else {
            *reinterpret_cast<uint32_t*>(col0 + 0 * LROW) = nic_pack_bf16x2(rb[0].x, rb[1].x);
            *reinterpret_cast<uint32_t*>(col0 + 1 * LROW) = nic_pack_bf16x2(rb[0].y, rb[1].y);
            *reinterpret_cast<uint32_t*>(col0 + 2 * LROW) = nic_pack_bf16x2(rb[0].z, rb[1].z);
            *reinterpret_cast<uint32_t*>(col0 + 3 * LROW) = nic_pack_bf16x2(rb[0].w, rb[1].w);
        }
    };

    f32x16 acc[MT][NT];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j) acc[i][j] = f32x16{};

    const int nk = p.K / BK;
    load(0);
    store(0);
    __syncthreads();
    for (int kt = 0; kt < nk; ++kt) {
        const int cur = kt & 1;
        if (kt + 1 < nk) load((kt + 1) * BK);   // next tile in flight behind this tile's MFMAs
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            bf16x8 a[MT], b[NT];
#pragma unroll
            for (int i = 0; i < MT; ++i)
                a[i] = *reinterpret_cast<const bf16x8*>(&sA[cur][(wm * MT * 32 + i * 32 + li) * LROW + s * 16 + h * 8]);
#pragma unroll
            for (int j = 0; j < NT; ++j)
                b[j] = *reinterpret_cast<const bf16x8*>(&sB[cur][(wn * NT * 32 + j * 32 + li) * LROW + s * 16 + h * 8]);
#pragma unroll
            for (int i = 0; i < MT; ++i)
#pragma unroll
                for (int j = 0; j < NT; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[i], b[j], acc[i][j], 0, 0, 0);
        }
        if (kt + 1 < nk) store(cur ^ 1);   // (buffer cur ^ 1 was last read before the previous barrier)
        __syncthreads();
    }

#pragma unroll
    for (int j = 0; j < NT; ++j) {
        const int col = c0 + wn * NT * 32 + j * 32 + li;
        if (col >= p.ncols) continue;
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = m0 + wm * MT * 32 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
                if (row >= p.M) continue;
                const int64_t off = (int64_t)row * p.ldb + col;
                float y = acc[i][j][r];
                if (EPI == EPI_BIAS_ACT) {
                    if (p.bias) y += p.bias[row];
                    if (p.act == NIC_ACT_ELU) y = elu_f(y);
                } else {
                    if (p.Hprev && p.act == NIC_ACT_ELU) y *= elu_grad_from_out(p.Hprev[off]);
                    if (p.accumulate) y += p.C[off];
                }
                p.C[off] = y;
            }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// wgrad kernel: slab[slot][n][k] += sum over the slot's (period, scenario) range of bf16(dY[n][b]) bf16(X[k][b]);
// column K += the FP32 sum of dY[n][b] (tiles of the first column block).  slot = period group * scen_splits + scenario split.
// ---------------------------------------------------------------------------------------------------------------
struct WgParams {
    const float* dY;  // [N][ldb] (period t: + t * pstride_dy)
    const float* X;   // [K][ldb] (period t: + t * pstride_x)
    float* slab;      // [slots][N][lds]
    int64_t lds_, ldb;
    int N, K, nB, chunk;              // chunk: scenarios per split (multiple of 32)
    int n_periods;
    int64_t pstride_dy, pstride_x;
    int flush;                        // periods between adds of the accumulators to the slab (~8k terms per partial sum)
    int scen_splits, ppg;             // slot factors; periods per group
};

// NCH float4 chunks per thread of a [rows][32 scenarios] tile (thread t: row (t + 256 i) >> 3, scenarios b0 + 4 ((t + 256 i) & 7));
// rows >= nrows and scenarios >= b_end read as 0 (the columns past b_end hold other splits' or padding values)
template <int NCH>
__device__ __forceinline__ void load_rows(const float* base, int64_t ldb, int nrows, int row0, int b0, int b_end, float4 (&dst)[NCH]) {
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
        const int idx = threadIdx.x + kThreads * i, row = row0 + (idx >> 3), b = b0 + (idx & 7) * 4;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (row < nrows) {
            const float* src = base + (int64_t)row * ldb + b;
            if (b + 3 < b_end) v = *reinterpret_cast<const float4*>(src);
            else {   // last, partial scenario tile of the chunk
                if (b + 0 < b_end) v.x = src[0];
                if (b + 1 < b_end) v.y = src[1];
                if (b + 2 < b_end) v.z = src[2];
            }
        }
        dst[i] = v;
    }
}

template <int MT, int NT>
__global__ __launch_bounds__(kThreads) void bf16_wgrad_kernel(WgParams p) {
    constexpr int BM = 2 * MT * 32, BN = 2 * NT * 32;
    constexpr int A_CH = BM * 8 / kThreads, B_CH = BN * 8 / kThreads;   // float4 chunks per thread per tile
    __shared__ __attribute__((aligned(16))) __bf16 sA[2][BM * LROW];
    __shared__ __attribute__((aligned(16))) __bf16 sB[2][BN * LROW];

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, wm = wave >> 1, wn = wave & 1;
    const int li = lane & 31, h = lane >> 5;
    const int tiles_m = (p.N + BM - 1) / BM, tiles_n = (p.K + BN - 1) / BN;
    const int id = xcd_swizzle(blockIdx.x, gridDim.x);
    const int slot = id / (tiles_m * tiles_n), tile = id % (tiles_m * tiles_n);
    const int n0 = (tile % tiles_m) * BM, k0 = (tile / tiles_m) * BN;
    const int ss = slot % p.scen_splits, grp = slot / p.scen_splits;
    const int b_begin = ss * p.chunk, t_begin = grp * p.ppg;
    if (b_begin >= p.nB || t_begin >= p.n_periods) return;   // (an unused slot: left untouched)
    const int b_end = min(b_begin + p.chunk, p.nB), t_end = min(t_begin + p.ppg, p.n_periods);
    const int nbt = (b_end - b_begin + BK - 1) / BK, ntiles = (t_end - t_begin) * nbt;
    const bool bias_tile = k0 == 0;
    float* out = p.slab + (int64_t)slot * p.N * p.lds_;

    float4 ra[A_CH], rb[B_CH];
    float rsum[A_CH];
#pragma unroll
    for (int i = 0; i < A_CH; ++i) rsum[i] = 0.f;
    auto load = [&](int it) {
        const int tp = t_begin + it / nbt, b0 = b_begin + (it % nbt) * BK;
        load_rows<A_CH>(p.dY + tp * p.pstride_dy, p.ldb, p.N, n0, b0, b_end, ra);
        load_rows<B_CH>(p.X + tp * p.pstride_x, p.ldb, p.K, k0, b0, b_end, rb);
        if (bias_tile) {
#pragma unroll
            for (int i = 0; i < A_CH; ++i) rsum[i] += (ra[i].x + ra[i].y) + (ra[i].z + ra[i].w);
        }
    };
    auto store = [&](int buf) {
#pragma unroll
        for (int i = 0; i < A_CH; ++i) {
            const int idx = t + kThreads * i;
            *reinterpret_cast<uint2*>(&sA[buf][(idx >> 3) * LROW + (idx & 7) * 4]) = cvt4(ra[i]);
        }
#pragma unroll
        for (int i = 0; i < B_CH; ++i) {
            const int idx = t + kThreads * i;
            *reinterpret_cast<uint2*>(&sB[buf][(idx >> 3) * LROW + (idx & 7) * 4]) = cvt4(rb[i]);
        }
    };

    f32x16 acc[MT][NT];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j) acc[i][j] = f32x16{};
    auto flush = [&]() {
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            const int col = k0 + wn * NT * 32 + j * 32 + li;
#pragma unroll
            for (int i = 0; i < MT; ++i)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = n0 + wm * MT * 32 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
                    if (row < p.N && col < p.K) out[(int64_t)row * p.lds_ + col] += acc[i][j][r];
                }
        }
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
            for (int j = 0; j < NT; ++j) acc[i][j] = f32x16{};
    };

    // partial sums go to the slab every `flush` periods; the owner workgroup is the only writer of its slab tile
    const int tiles_per_flush = p.flush * nbt;
    for (int f0 = 0; f0 < ntiles; f0 += tiles_per_flush) {
        const int f1 = min(f0 + tiles_per_flush, ntiles);
        load(f0);
        store(0);
        __syncthreads();
        for (int it = f0; it < f1; ++it) {
            const int cur = (it - f0) & 1;
            if (it + 1 < f1) load(it + 1);
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                bf16x8 a[MT], b[NT];
#pragma unroll
                for (int i = 0; i < MT; ++i)
                    a[i] = *reinterpret_cast<const bf16x8*>(&sA[cur][(wm * MT * 32 + i * 32 + li) * LROW + s * 16 + h * 8]);
#pragma unroll
                for (int j = 0; j < NT; ++j)
                    b[j] = *reinterpret_cast<const bf16x8*>(&sB[cur][(wn * NT * 32 + j * 32 + li) * LROW + s * 16 + h * 8]);
#pragma unroll
                for (int i = 0; i < MT; ++i)
#pragma unroll
                    for (int j = 0; j < NT; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[i], b[j], acc[i][j], 0, 0, 0);
            }
            if (it + 1 < f1) store(cur ^ 1);
            __syncthreads();
        }
        flush();
    }
    if (bias_tile) {   // the 8 lanes that share a dY row (consecutive lanes, q = idx & 7) add their FP32 sums
#pragma unroll
        for (int i = 0; i < A_CH; ++i) {
            float s = rsum[i];
            s += __shfl_xor(s, 1);
            s += __shfl_xor(s, 2);
            s += __shfl_xor(s, 4);
            const int row = n0 + ((t + kThreads * i) >> 3);
            if ((t & 7) == 0 && row < p.N) out[(int64_t)row * p.lds_ + p.K] += s;
        }
    }
}

bool aligned16(const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; }

template <int EPI>
int launch_wx(const WxParams& p, hipStream_t s) {
    const nic::Bf16WxTile t = nic::bf16_wx_tile(p.M, p.ncols, nic::cu_count());   // 128 x 128 tiles for big launches, else 64 x 64
    nic::note_kernelf("bf16_wx_kernel<%d,%d,%d>", t.mt_nt, t.mt_nt, EPI);
    if (t.mt_nt == 2) hipLaunchKernelGGL((bf16_wx_kernel<2, 2, EPI>), dim3((unsigned)t.grid), dim3(kThreads), 0, s, p);
    else hipLaunchKernelGGL((bf16_wx_kernel<1, 1, EPI>), dim3((unsigned)t.grid), dim3(kThreads), 0, s, p);
    return 0;
}

// period_groups: slots are (scenario split, period group) pairs, else scenario splits; factors, chunk and flush: wgrad_plan.h
int wgrad_bf16(const float* dY, const float* X, float* slab, int64_t lds_, int32_t N, int32_t K, int32_t n_scenarios, int32_t ldb,
               int32_t n_slots, int32_t n_periods, int64_t pstride_dy, int64_t pstride_x, bool period_groups, void* stream,
               const char* who) {
    NIC_REQUIRE(dY && X && slab, "%s: null buffer", who);
    NIC_REQUIRE(nic_linear_bf16_ok(N, K), "%s: N and K must be multiples of 32 and >= 128 (%d x %d)", who, N, K);
    NIC_REQUIRE(lds_ >= K + 1 && n_slots >= 1, "%s: bad lds / n_splits (%lld / %d)", who, (long long)lds_, n_slots);
    NIC_REQUIRE(n_scenarios > 0 && ldb >= n_scenarios && ldb % 4 == 0, "%s: ldb (%d) must be a multiple of 4 and >= n_scenarios (%d)",
                who, ldb, n_scenarios);
    NIC_REQUIRE(aligned16(dY) && aligned16(X) && pstride_dy % 4 == 0 && pstride_x % 4 == 0,
                "%s: dY / X must be 16-byte aligned (period strides multiples of 4 elements)", who);
    const nic::WgradSlots slots = period_groups ? nic::period_factors(n_slots, n_scenarios, n_periods)
                                                : nic::scenario_slots(n_slots, n_scenarios, n_periods);
    WgParams p{dY, X, slab, lds_, ldb, N, K, n_scenarios, slots.chunk, n_periods, pstride_dy, pstride_x,
               nic::wgrad_flush_periods(slots.chunk), slots.scen_splits, slots.periods_per_group};
    const int tiles = ((N + 127) / 128) * ((K + 127) / 128);
    nic::note_kernel("bf16_wgrad_kernel<2,2>");
    hipLaunchKernelGGL((bf16_wgrad_kernel<2, 2>), dim3(tiles * slots.scen_splits * slots.groups), dim3(kThreads), 0,
                       nic::as_stream(stream), p);
    return nic::check_launch(who);
}

}  // namespace

extern "C" {

int nic_linear_bf16_ok(int32_t N, int32_t K) { return N >= 128 && K >= 128 && N % 32 == 0 && K % 32 == 0; }

int nic_linear_bf16_fwd(const uint16_t* W, int64_t ldw, const float* bias, const float* X, float* Y, int32_t N, int32_t K,
                        int32_t n_scenarios, int32_t ldb, int32_t act, void* stream) {
    NIC_REQUIRE(W && X && Y, "nic_linear_bf16_fwd: null buffer");
    NIC_REQUIRE(nic_linear_bf16_ok(N, K), "nic_linear_bf16_fwd: N and K must be multiples of 32 and >= 128 (%d x %d)", N, K);
    NIC_REQUIRE(ldw >= K && ldw % 8 == 0, "nic_linear_bf16_fwd: ldw (%lld) must be >= K and a multiple of 8", (long long)ldw);
    NIC_REQUIRE(act == NIC_ACT_NONE || act == NIC_ACT_ELU, "nic_linear_bf16_fwd: unknown activation %d", act);
    NIC_REQUIRE(n_scenarios > 0 && ldb >= n_scenarios && ldb % 4 == 0,
                "nic_linear_bf16_fwd: ldb (%d) must be a multiple of 4 and >= n_scenarios (%d)", ldb, n_scenarios);
    NIC_REQUIRE(aligned16(W) && aligned16(X) && aligned16(Y), "nic_linear_bf16_fwd: W / X / Y must be 16-byte aligned");
    WxParams p{reinterpret_cast<const __bf16*>(W), ldw, X, Y, bias, nullptr, N, K, (n_scenarios + 3) / 4 * 4, ldb, act, 0};
    launch_wx<EPI_BIAS_ACT>(p, nic::as_stream(stream));
    return nic::check_launch("nic_linear_bf16_fwd");
}

int nic_linear_bf16_dgrad(const uint16_t* Wt, int64_t ldwt, const float* dY, const float* Hprev, float* dX, int32_t N, int32_t K,
                          int32_t n_scenarios, int32_t ldb, int32_t act_prev, int32_t accumulate, void* stream) {
    NIC_REQUIRE(Wt && dY && dX, "nic_linear_bf16_dgrad: null buffer");
    NIC_REQUIRE(nic_linear_bf16_ok(N, K), "nic_linear_bf16_dgrad: N and K must be multiples of 32 and >= 128 (%d x %d)", N, K);
    NIC_REQUIRE(ldwt >= N && ldwt % 8 == 0, "nic_linear_bf16_dgrad: ldwt (%lld) must be >= N and a multiple of 8", (long long)ldwt);
    NIC_REQUIRE(n_scenarios > 0 && ldb >= n_scenarios && ldb % 4 == 0,
                "nic_linear_bf16_dgrad: ldb (%d) must be a multiple of 4 and >= n_scenarios (%d)", ldb, n_scenarios);
    NIC_REQUIRE(aligned16(Wt) && aligned16(dY) && aligned16(dX), "nic_linear_bf16_dgrad: Wt / dY / dX must be 16-byte aligned");
    // dX[K][b] = Wt[K][N] * dY[N][b]: output rows = K, contraction = N
    WxParams p{reinterpret_cast<const __bf16*>(Wt), ldwt, dY, dX, nullptr, Hprev, K, N, (n_scenarios + 3) / 4 * 4, ldb, act_prev,
               accumulate};
    launch_wx<EPI_DGRAD>(p, nic::as_stream(stream));
    return nic::check_launch("nic_linear_bf16_dgrad");
}

int nic_linear_bf16_wgrad(const float* dY, const float* X, float* slab, int64_t lds_, int32_t N, int32_t K, int32_t n_scenarios,
                          int32_t ldb, int32_t n_splits, void* stream) {
    return wgrad_bf16(dY, X, slab, lds_, N, K, n_scenarios, ldb, n_splits, 1, 0, 0, false, stream, "nic_linear_bf16_wgrad");
}

int nic_linear_bf16_wgrad_periods(const float* dY, const float* X, float* slab, int64_t lds_, int32_t N, int32_t K,
                                  int32_t n_scenarios, int32_t ldb, int32_t n_splits, int32_t n_periods, int64_t period_stride_dy,
                                  int64_t period_stride_x, void* stream) {
    NIC_REQUIRE(n_periods >= 1 && n_splits >= 1, "nic_linear_bf16_wgrad_periods: n_periods and n_splits must be >= 1");
    // last period first, as nic_linear_wgrad_periods (autograd's order: the small terms are summed before the large ones)
    if (n_periods > 1) {
        dY += (int64_t)(n_periods - 1) * period_stride_dy;
        X += (int64_t)(n_periods - 1) * period_stride_x;
        period_stride_dy = -period_stride_dy;
        period_stride_x = -period_stride_x;
    }
    return wgrad_bf16(dY, X, slab, lds_, N, K, n_scenarios, ldb, n_splits, n_periods, period_stride_dy, period_stride_x, true,
                      stream, "nic_linear_bf16_wgrad_periods");
}
}
