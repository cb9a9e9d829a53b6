// Policy-MLP layers on the gfx950 FP32 matrix cores (v_mfma_f32_32x32x2_f32: exact f32 products and accumulation,
// bit-for-bit an fmaf chain, 256 FLOP/clk/CU = 157 TFLOP/s peak) — the reference's aten::addmm/mm + elu /
// elu_backward (neural_networks.py:80-106) re-designed around feature-major activations.
//
// Formulation.  Activations are stored feature-major, X[k][b] (scenario index contiguous), so
//     forward   Y[n][b]  = act( sum_k W[n][k]  X[k][b] + bias[n] )         "wx" kernel, A = W   (N x K)
//     dgrad     dX[k][b] = ( sum_n Wt[k][n] dY[n][b] ) * act'(H[k][b])     "wx" kernel, A = W^T (K x N)
//     wgrad     dW[n][k] += sum_b dY[n][b] X[k][b]                          "wgrad" kernel, contraction over scenarios
// In the wx kernel the MFMA's lane index is the scenario: the B operand (lane l holds B[k=l>>5][j=l&31]) and the
// C/D tile (col = lane&31) are read / written as contiguous 128-byte scenario runs, i.e. coalesced with no
// transposition anywhere between the env-step kernels and the GEMMs.
//
// Production kernels (16-byte aligned operands — everything the rollout engine allocates):
//   gemm_wx_dma_kernel     forward + dgrad; 128 x 128 x 32 block tile of 8 waves (2 x 4, wave tile 64 x 32), two workgroups
//                          co-resident per CU; 64 x 128 (8 waves) and 32 x 128 (4 waves) for small launches / thin or ragged
//                          outputs (pick_wx_tile in wx_plan.h; round 4: co-resident workgroups beat one 256 x 256 workgroup per CU)
//   gemm_wgrad_dma_kernel  weight gradient, 128 x 256 output tile per (scenario chunk, period group), 8 waves (2 x 4)
//   both: tiles go HBM/L2 -> LDS by `buffer_load_dwordx4 ... lds` (no VGPR round trip), double-buffered, one barrier per
//   k tile; A-style tiles [rows][32] are unpadded with a 16-byte-chunk XOR swizzle applied on the DMA source address
//   and on the ds_read_b128 fragment reads; the [32][BN] B tile of the wx kernel is linear (ds_read_b32 rows);
//   epilogues are staged through the dead LDS tiles and leave as whole-row float4 accesses; logical tile order is
//   XCD-aware.
//   k order : within a 16-deep k group, MFMA step kk consumes k = kk (lanes 0-31) and k = 8+kk (lanes 32-63), so a
//             lane's eight A values of a group are CONTIGUOUS in LDS (two ds_read_b128) — summation order over k is
//             free because parity is defined to 1e-5, not bitwise, for the policy GEMMs.
// Fallback kernels (gemm_wx_kernel, gemm_wgrad_kernel): register-staged, per-element guards, for unaligned operands,
// scenario counts that are not a multiple of 32, and the thin layers of the weight gradient.
// Dispatch: forward / dgrad (kernel, grid, reported name) in wx_plan.h, launched by dispatch_wx below; the weight gradient (kernel,
// slab slots, chunk, flush, launches) in wgrad_plan.h.  Both headers are plain C++ that the host tests run without a GPU.
// Roofline: MFMA-bound.  Measured on MI355X (512 x 512 x 65,536): 102-114 TFLOP/s; MFMA pipe 70 % busy at a 2.26 GHz
// sustained clock (profiles/r01_gemm_pmc_dma256.txt); the remainder is the per-tile DMA wait + barrier (a no-DMA timing
// build runs 117 TFLOP/s) and the unoverlapped prologue / epilogue of a 1-workgroup-per-CU kernel.
#include <type_traits>
#include <stdlib.h>
#include <string.h>

#include "linear_models_plan.h"
#include "nic_common.h"
#include "wgrad_plan.h"
#include "wx_plan.h"

namespace {

using f32x16 = __attribute__((ext_vector_type(16))) float;

constexpr int BK = 32;       // k depth of one LDS tile
constexpr int LDA_S = 36;    // padded LDS row (floats) for k-contiguous tiles
constexpr int kThreads = 256;

enum { EPI_BIAS_ACT = 0, EPI_DGRAD = 1 };
const char* epi_name(int epi) { return epi == EPI_BIAS_ACT ? "EPI_BIAS_ACT" : "EPI_DGRAD"; }

// In-kernel timestamps and timing-only switches (tuning build only: tools/gemm_stamp_probe.py compiles its own copy of the
// library with -DNIC_TUNING_BUILD; the product library contains none of this).  Slot s of workgroup w: {s_memtime, 100 MHz wall
// clock} at kernel entry (0), in front of the k loop (1), behind it (2) and at exit (3).
#ifdef NIC_TUNING_BUILD
__device__ unsigned long long* g_nic_stamps = nullptr;
#define NIC_STAMP(slot)                                                                  \
    do {                                                                                 \
        if (g_nic_stamps != nullptr && threadIdx.x == 0) {                               \
            g_nic_stamps[(blockIdx.x * 4 + (slot)) * 2] = __builtin_readcyclecounter();  \
            g_nic_stamps[(blockIdx.x * 4 + (slot)) * 2 + 1] = wall_clock64();            \
        }                                                                                \
    } while (0)
#define NIC_TUNE(bit) (p.tune & (bit))
#else
#define NIC_STAMP(slot) do { } while (0)
#define NIC_TUNE(bit) false
#endif

struct WxParams {
    const float* A;      // [M][lda]
    int64_t lda;
    const float* Bm;     // [K][ldb]
    float* C;            // [M][ldb]
    const float* bias;   // [M] or null            (EPI_BIAS_ACT)
    const float* Hprev;  // [M][ldb] or null        (EPI_DGRAD: multiply by act'(Hprev))
    int M, K, ncols;     // ncols = columns to produce (multiple of 4, <= ldb)
    int64_t ldb;
    int act;             // NIC_ACT_*
    int accumulate;      // EPI_DGRAD: C += result
    int tune;            // tuning build only, timing experiments (results invalid): 1 = no A-tile copies inside the k loop,
                         // 2 = no B-tile copies, 4 = no barrier per k tile, 32 = s_setprio 1 for waves 4-7 (valid results),
                         // 8 = dgrad without the Hprev prefetch, 16 = stamp 1 behind the plain k tiles, 64 = forward epilogue
                         // straight from the accumulators, 128 = 256 x 256 tiling whatever the shape (8-128: valid results)
    // model form (MODELS instantiations, grid y = model): floats between two models' A, Bm (0: one shared input), C and bias
    int64_t mA, mB, mC, mBias;
};
// what a MASKED instantiation takes: the same, and the active-model mask (int32 [models]; NULL: every model runs) BEHIND it - every
// other instantiation keeps WxParams, its kernel-argument bytes and its instruction stream
struct WxModelParams : WxParams { const int32_t* active; };
template <bool MASKED> using WxArgs = std::conditional_t<MASKED, WxModelParams, WxParams>;

// Model forms (nic_linear_*_models; csrc/linear_models_plan.h).  A MODELS instantiation advances its operand pointers once, at
// entry, by blockIdx.y x the model stride (64-bit) and then runs the single-model body unchanged: every offset formed afterwards is
// an offset inside one model's slice, and grid x is the single-model launch's.  xcd_swizzle(blockIdx.x, gridDim.x) keeps working per
// model row; as workgroups are dealt over the XCDs in linear order of (y, x), the XCD a logical tile lands on may rotate from model
// to model when gridDim.x is not a multiple of 8 - a locality matter only (a model's tiles still share their XCD ranges).
// The active-model mask (the *_models_active entry points): a MASKED instantiation (with MODELS) asks model_stopped FIRST and returns
// at entry for a model whose entry is zero - ahead of the advance, every load and store, LDS and barrier.  Workgroup id and a kernel
// argument: the test is wave- and workgroup-uniform, one scalar load and a branch.  DECISION: MASKED twins of the MODELS
// instantiations, launched by the _active entry points only, as for the rollout kernels.  The test put into the MODELS
// instantiations themselves (NULL from the entry points without a mask) left every VGPR / AGPR / spill count alone but moved
// wgrad_small_kernel<2..4, true> from 50 to 54 SGPRs, and the rule was "no register count moves": with twins the single-model AND the
// unmasked model instantiations keep their parameter types and compile to the instruction streams they had.
template <class Params> __device__ __forceinline__ bool model_stopped(const Params& p) {
    return !nic::linear_model_runs(p.active, blockIdx.y);
}
__device__ __forceinline__ void advance_models(WxParams& p) {
    p.A += nic::linear_model_offset(blockIdx.y, p.mA);
    p.Bm += nic::linear_model_offset(blockIdx.y, p.mB);
    p.C += nic::linear_model_offset(blockIdx.y, p.mC);
    if (p.bias) p.bias += nic::linear_model_offset(blockIdx.y, p.mBias);
}

// ELU.  libm's expm1f is ~40 VALU instructions and the epilogue applies it to every output element (33.5 M per 512-wide
// layer at 65,536 scenarios: ~20 us of pure VALU per launch); this branch-free form is a 6-term series near zero (relative
// error < 2e-7 for x > -0.35) and exp(x) - 1 on the hardware exponential below that (absolute error ~1e-7).
__device__ __forceinline__ float elu_f(float x) {
    const float xn = fminf(x, 0.f);
    const float series =
        xn * fmaf(xn, fmaf(xn, fmaf(xn, fmaf(xn, fmaf(xn, 1.f / 720.f, 1.f / 120.f), 1.f / 24.f), 1.f / 6.f), 0.5f), 1.f);
    const float viaexp = __expf(xn) - 1.f;
    const float neg = xn > -0.35f ? series : viaexp;
    return x > 0.f ? x : neg;
}
// derivative of ELU expressed with its OUTPUT y: x > 0 -> 1, else exp(x) = y + 1
__device__ __forceinline__ float elu_grad_from_out(float y) { return y > 0.f ? 1.f : y + 1.f; }

// ---- tile loaders (global -> registers) -----------------------------------------------------------------------
// k-contiguous tile: ROWS x 32 floats, element (r, k) at src[(row0 + r) * ld + k0 + k]; rows >= nrows and k >= kmax
// are zero-filled.  Each thread moves ROWS/32 float4 (thread t: row = t/8 + 32*i, k4 = t%8).
template <int ROWS>
struct KTile {
    static constexpr int N4 = ROWS / 32;
    float4 v[N4];
    __device__ __forceinline__ void load(const float* __restrict__ src, int64_t ld, int row0, int nrows, int k0, int kmax,
                                         bool vec_ok, int ones_row = -1, int ones_cols = 0) {
        const int t = threadIdx.x;
        const int k = k0 + (t & 7) * 4;
#pragma unroll
        for (int i = 0; i < N4; ++i) {
            const int r = row0 + (t >> 3) + 32 * i;
            float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
            if (r < nrows) {
                const float* p = src + (int64_t)r * ld + k;
                if (vec_ok && k + 3 < kmax) {
                    x = *reinterpret_cast<const float4*>(p);
                } else {
                    if (k + 0 < kmax) x.x = p[0];
                    if (k + 1 < kmax) x.y = p[1];
                    if (k + 2 < kmax) x.z = p[2];
                    if (k + 3 < kmax) x.w = p[3];
                }
            } else if (r == ones_row) {  // virtual row of ones: its wgrad column is the bias gradient
                x.x = k + 0 < ones_cols ? 1.f : 0.f;
                x.y = k + 1 < ones_cols ? 1.f : 0.f;
                x.z = k + 2 < ones_cols ? 1.f : 0.f;
                x.w = k + 3 < ones_cols ? 1.f : 0.f;
            }
            v[i] = x;
        }
    }
    __device__ __forceinline__ void store(float* lds /* [ROWS][LDA_S] */) const {
        const int t = threadIdx.x;
#pragma unroll
        for (int i = 0; i < N4; ++i)
            *reinterpret_cast<float4*>(lds + ((t >> 3) + 32 * i) * LDA_S + (t & 7) * 4) = v[i];
    }
};

// column-contiguous tile: 32 (k) x COLS floats, element (k, c) at src[(k0 + k) * ld + c0 + c]; k >= kmax and
// c >= ncols zero-filled.  Thread t: c4 = t % (COLS/4), k = t / (COLS/4) + (256*4/COLS) * i.
template <int COLS>
struct CTile {
    static constexpr int TPR = COLS / 4;            // threads per row
    static constexpr int RPI = kThreads / TPR;      // rows per iteration
    static constexpr int N4 = BK / RPI;
    float4 v[N4];
    __device__ __forceinline__ void load(const float* __restrict__ src, int64_t ld, int k0, int kmax, int c0, int ncols) {
        const int t = threadIdx.x;
        const int c = c0 + (t % TPR) * 4;
#pragma unroll
        for (int i = 0; i < N4; ++i) {
            const int k = k0 + t / TPR + RPI * i;
            float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
            if (k < kmax && c < ncols) x = *reinterpret_cast<const float4*>(src + (int64_t)k * ld + c);
            v[i] = x;
        }
    }
    __device__ __forceinline__ void store(float* lds /* [32][COLS] */) const {
        const int t = threadIdx.x;
#pragma unroll
        for (int i = 0; i < N4; ++i)
            *reinterpret_cast<float4*>(lds + (t / TPR + RPI * i) * COLS + (t % TPR) * 4) = v[i];
    }
};

// ---- branch-free tile loaders (buffer loads: hardware range check returns 0 past num_records) ------------------------
// The guarded loaders above branch per element and hipcc serialises their loads behind s_waitcnt; in the k loop that
// stalls every tile.  When the operand rows are 16-byte aligned the tile is fetched with raw buffer loads instead: rows
// past the end of the matrix are out of range of the descriptor and read as 0.0 without a branch, so the loads of a
// tile issue back to back.  Columns past K inside an A row read whatever follows (row padding or the next row — finite
// weights) and are multiplied by B rows that ARE out of range (zero), so no k guard is needed either.
__device__ __forceinline__ float4 buf_load4(__amdgpu_buffer_rsrc_t rsrc, int byte_off) {
    return __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rsrc, byte_off, 0, 0));
}
__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const float* p, int64_t n_floats) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p), 0, (int)(n_floats * 4), 0x00020000);
}

// LDS-DMA issued from inline asm.  With the builtin (__builtin_amdgcn_raw_ptr_buffer_load_lds) hipcc cannot prove that the
// ds_reads of pipeline stage `cur` do not alias the DMA writes into stage `cur ^ 1` (same __shared__ array) and puts an
// s_waitcnt vmcnt(0) in front of the first fragment read of EVERY tile: the copy it was meant to overlap is waited for
// before the MFMAs start (measured: 13 % of the kernel).  An asm statement is outside hipcc's vmcnt bookkeeping; the
// kernels drain the DMA themselves (dma_wait) right before the barrier that publishes the tile.
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ u32x4 make_desc(const float* p, int64_t n_floats) {
    const uint64_t a = reinterpret_cast<uint64_t>(p);
    u32x4 d;
    d.x = (unsigned)a;
    d.y = (unsigned)(a >> 32) & 0xffffu;  // stride 0: raw buffer
    d.z = (unsigned)(n_floats * 4);       // num_records in bytes: loads past it return 0
    d.w = 0x00020000u;
    return d;
}
// lds_addr: wave-uniform LDS byte address; lane l's 16 bytes land at lds_addr + 16 * l.  M0 is saved / restored inside the
// statement (it is compiler-reserved); s_nop 0 covers the SALU-write-M0 -> LDS-DMA hazard.
__device__ __forceinline__ void dma16(u32x4 desc, int voff, unsigned lds_addr) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, 0 offen lds\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(voff), "s"(desc), "s"(lds_addr)
                 : "memory");
}
__device__ __forceinline__ void dma_wait() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

template <int ROWS>
struct KTileBuf {
    static constexpr int N4 = ROWS / 32;
    float4 v[N4];
    int off[N4];  // byte offsets of this thread's float4s in the current tile
    __device__ __forceinline__ void init(int64_t ld, int row0, int k0) {
        const int t = threadIdx.x;
#pragma unroll
        for (int i = 0; i < N4; ++i) off[i] = (int)((((int64_t)row0 + (t >> 3) + 32 * i) * ld + k0 + (t & 7) * 4) * 4);
    }
    __device__ __forceinline__ void load(__amdgpu_buffer_rsrc_t rsrc) {
#pragma unroll
        for (int i = 0; i < N4; ++i) v[i] = buf_load4(rsrc, off[i]);
    }
    __device__ __forceinline__ void advance(int tiles = 1) {
#pragma unroll
        for (int i = 0; i < N4; ++i) off[i] += tiles * BK * 4;
    }
    // wgrad: zero the scenarios at or past b_end; row `ones_row` is a virtual row of ones (bias gradient column)
    __device__ __forceinline__ void mask_cols(int b0, int b_end, int row0, int ones_row) {
        const int t = threadIdx.x;
        const int b = b0 + (t & 7) * 4;
#pragma unroll
        for (int i = 0; i < N4; ++i) {
            const bool one = (row0 + (t >> 3) + 32 * i) == ones_row;
            float4 x = v[i];
            x.x = b + 0 < b_end ? (one ? 1.f : x.x) : 0.f;
            x.y = b + 1 < b_end ? (one ? 1.f : x.y) : 0.f;
            x.z = b + 2 < b_end ? (one ? 1.f : x.z) : 0.f;
            x.w = b + 3 < b_end ? (one ? 1.f : x.w) : 0.f;
            v[i] = x;
        }
    }
    __device__ __forceinline__ void store(float* lds) const {
        const int t = threadIdx.x;
#pragma unroll
        for (int i = 0; i < N4; ++i)
            *reinterpret_cast<float4*>(lds + ((t >> 3) + 32 * i) * LDA_S + (t & 7) * 4) = v[i];
    }
};

// Workgroups are dealt round-robin over the 8 XCDs (each with a private L2).  Remap the linear workgroup id so that every
// XCD gets a CONTIGUOUS range of logical tiles: the tiles that share an operand panel (the row tiles of one scenario
// panel in the wx kernel, the 16 output tiles of one scenario chunk in the wgrad kernel) then run on one XCD at about
// the same time and the panel is fetched from HBM once instead of once per XCD.  Bijective for any grid size.
__device__ __forceinline__ int xcd_swizzle(int bid, int nwg) {
    const int q = nwg >> 3, r = nwg & 7, xcd = bid & 7, idx = bid >> 3;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
}

// eight k-contiguous operand values of one lane for k group g (see "k order" above)
__device__ __forceinline__ void read_frag8(const float* lds_row, int g, int h, float (&f)[8]) {
    const float4 lo = *reinterpret_cast<const float4*>(lds_row + g * 16 + h * 8);
    const float4 hi = *reinterpret_cast<const float4*>(lds_row + g * 16 + h * 8 + 4);
    f[0] = lo.x; f[1] = lo.y; f[2] = lo.z; f[3] = lo.w;
    f[4] = hi.x; f[5] = hi.y; f[6] = hi.z; f[7] = hi.w;
}

// ---------------------------------------------------------------------------------------------------------------
// wx kernel, guarded form: C[M][ncols] = epilogue( A[M][K] * Bm[K][ncols] ) for operands that are NOT 16-byte aligned /
// row-padded (e.g. an unpadded [N][51] weight handed over by HipLinear).  Register-staged double buffering with
// per-element guards; correctness path, not the performance path (aligned operands use gemm_wx_dma_kernel below).
// ---------------------------------------------------------------------------------------------------------------
template <int WAVES_M, int WAVES_N, int MT, int NT, int EPI, bool MODELS = false, bool MASKED = false>
__global__ __launch_bounds__(kThreads) void gemm_wx_kernel(WxArgs<MASKED> p) {
    if constexpr (MODELS) {
        if constexpr (MASKED) {
            if (model_stopped(p)) return;
        }
        advance_models(p);
    }
    constexpr int BM = WAVES_M * MT * 32;
    constexpr int BN = WAVES_N * NT * 32;
    static_assert(WAVES_M * WAVES_N == 4, "4 waves per workgroup");
    constexpr int STAGE = BM * LDA_S + BK * BN;  // floats per pipeline stage: A tile then B tile
    __shared__ __attribute__((aligned(16))) float lds[2 * STAGE];

    const int tiles_m = (p.M + BM - 1) / BM;
    const int m0 = (blockIdx.x % tiles_m) * BM;
    const int c0 = (blockIdx.x / tiles_m) * BN;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wm = wave / WAVES_N, wn = wave % WAVES_N;
    const int li = lane & 31, h = lane >> 5;
    const bool vecA = (p.lda % 4 == 0) && ((reinterpret_cast<uintptr_t>(p.A) & 15) == 0);

    f32x16 acc[MT][NT];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    const int nk = (p.K + BK - 1) / BK;
    KTile<BM> ta;
    CTile<BN> tb;
    ta.load(p.A, p.lda, m0, p.M, 0, p.K, vecA);
    tb.load(p.Bm, p.ldb, 0, p.K, c0, p.ncols);
    ta.store(lds);
    tb.store(lds + BM * LDA_S);
    __syncthreads();
    for (int kt = 0; kt < nk; ++kt) {
        const int cur = kt & 1;
        if (kt + 1 < nk) {
            ta.load(p.A, p.lda, m0, p.M, (kt + 1) * BK, p.K, vecA);
            tb.load(p.Bm, p.ldb, (kt + 1) * BK, p.K, c0, p.ncols);
        }
        const float* a_base = lds + cur * STAGE + (wm * MT * 32 + li) * LDA_S;
        const float* b_base = lds + cur * STAGE + BM * LDA_S + wn * NT * 32 + li;
#pragma unroll
        for (int g = 0; g < 2; ++g) {
            float a[MT][8];
#pragma unroll
            for (int i = 0; i < MT; ++i) read_frag8(a_base + i * 32 * LDA_S, g, h, a[i]);
#pragma unroll
            for (int kk = 0; kk < 8; ++kk) {
                float b[NT];
#pragma unroll
                for (int j = 0; j < NT; ++j) b[j] = b_base[(g * 16 + h * 8 + kk) * BN + j * 32];
#pragma unroll
                for (int i = 0; i < MT; ++i)
#pragma unroll
                    for (int j = 0; j < NT; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i][kk], b[j], acc[i][j], 0, 0, 0);
            }
        }
        if (kt + 1 < nk) {
            ta.store(lds + (cur ^ 1) * STAGE);
            tb.store(lds + (cur ^ 1) * STAGE + BM * LDA_S);
        }
        __syncthreads();
    }

    // epilogue straight from the accumulators: C/D layout col = lane & 31, row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)
#pragma unroll
    for (int i = 0; i < MT; ++i) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = m0 + (wm * MT + i) * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
            if (row >= p.M) continue;
            float bias = 0.f;
            if (EPI == EPI_BIAS_ACT && p.bias) bias = p.bias[row];
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                const int col = c0 + (wn * NT + j) * 32 + li;
                if (col >= p.ncols) continue;
                const int64_t off = (int64_t)row * p.ldb + col;
                float y = acc[i][j][r];
                if (EPI == EPI_BIAS_ACT) {
                    y += bias;
                    if (p.act == NIC_ACT_ELU) y = elu_f(y);
                } else {
                    if (p.Hprev && p.act == NIC_ACT_ELU) y *= elu_grad_from_out(p.Hprev[off]);
                    if (p.accumulate) y += p.C[off];
                }
                p.C[off] = y;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// wx kernel, LDS-DMA form (the production path): tiles go HBM/L2 -> LDS with `buffer_load_dwordx4 ... lds`, no VGPR
// round trip and no ds_write.  Measured on MI355X at 512x512x65536: the register-staged loop spends 13 % of its time
// in the ds_write_b128 transfer and 5 % in the loads; both disappear here.
//   A tile [BM][32] floats, UNPADDED (a DMA wave-instruction writes 1 KiB linearly = 8 rows), 16-byte chunks XOR-
//     swizzled with ((row >> 1) & 7) on the SOURCE address; the ds_read_b128 fragment reads apply the same XOR, which
//     makes every 16-lane read group hit 16 distinct bank quads (rows r, r+1 differ in the 32-bank half).
//   B tile [32][BN] floats, linear (row reads by ds_read_b32 are conflict-free as they are).
//   Rows past the matrix end are out of range of the buffer descriptor: the DMA writes zeros, no branches.
// ---------------------------------------------------------------------------------------------------------------
template <int WAVES_M, int WAVES_N, int MT, int NT, int EPI, bool MODELS = false, bool MASKED = false>
__global__ __launch_bounds__(64 * WAVES_M * WAVES_N) void gemm_wx_dma_kernel(WxArgs<MASKED> p) {
#if defined(__HIP_DEVICE_COMPILE__)  // LDS address-space pointers only exist in the device pass
    if constexpr (MODELS) {
        if constexpr (MASKED) {
            if (model_stopped(p)) return;
        }
        advance_models(p);
    }
    constexpr int NW = WAVES_M * WAVES_N, NTHREADS = 64 * NW;
    constexpr int BM = WAVES_M * MT * 32;
    constexpr int BN = WAVES_N * NT * 32;
    static_assert(NW == 4 || NW == 8, "4 or 8 waves per workgroup");
    constexpr int A_FLOATS = BM * BK, B_FLOATS = BK * BN, STAGE = A_FLOATS + B_FLOATS;
    constexpr int LDC = BN + 4;
    // epilogue staging: the whole C tile if it fits next to nothing else, otherwise one wave-row (MT*32 rows) per pass
    constexpr int PASSES = (BM * LDC * 4 <= 72 * 1024) ? 1 : WAVES_M;
    constexpr int PASS_ROWS = BM / PASSES;
    constexpr int LDS_FLOATS = (2 * STAGE > PASS_ROWS * LDC) ? 2 * STAGE : PASS_ROWS * LDC;
    __shared__ __attribute__((aligned(16))) float lds[LDS_FLOATS];
    typedef __attribute__((address_space(3))) void* lds_ptr_t;

    NIC_STAMP(0);
    const int tiles_m = (p.M + BM - 1) / BM;
    const int tile = xcd_swizzle(blockIdx.x, gridDim.x);
    const int m0 = (tile % tiles_m) * BM;
    const int c0 = (tile / tiles_m) * BN;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wm = wave / WAVES_N, wn = wave % WAVES_N;
    const int li = lane & 31, h = lane >> 5;

    const u32x4 ra = make_desc(p.A, (int64_t)p.M * p.lda);
    const u32x4 rb = make_desc(p.Bm, (int64_t)p.K * p.ldb);
    const unsigned lds0 = (unsigned)(uintptr_t)(lds_ptr_t)lds;  // LDS byte address of the staging array
    constexpr int A_INSTR = BM / 8 / NW;           // 1-KiB DMA instructions per wave for the A tile (8 rows each)
    constexpr int B_INSTR = BN / 8 / NW;           // ... for the B tile (256/BN rows each)
    constexpr int B_LPR = BN / 4;                  // lanes per B row
    static_assert(A_INSTR >= 1 && B_INSTR >= 1 && B_LPR <= 64, "tile too small for this wave count");
    int offA[A_INSTR], offB[B_INSTR];
#pragma unroll
    for (int q = 0; q < A_INSTR; ++q) {
        const int row = (wave * A_INSTR + q) * 8 + (lane >> 3);
        const int chunk = (lane & 7) ^ ((row >> 1) & 7);  // LDS position (lane & 7) holds source chunk `chunk`
        offA[q] = (int)((((int64_t)m0 + row) * p.lda + chunk * 4) * 4);
    }
#pragma unroll
    for (int q = 0; q < B_INSTR; ++q) {
        const int row = (wave * B_INSTR + q) * (64 / B_LPR) + lane / B_LPR;
        offB[q] = (int)(((int64_t)row * p.ldb + c0 + (lane % B_LPR) * 4) * 4);
    }
    const int stepB = (int)(p.ldb * BK * 4);
    bool in_loop = false;  // (tuning build: the timing-only switches leave the prologue's copy alone)
    auto issue = [&](int stage) {
        const unsigned base = __builtin_amdgcn_readfirstlane(lds0 + (unsigned)(stage * STAGE) * 4u);
        const unsigned wbase_a = __builtin_amdgcn_readfirstlane(base + (unsigned)(wave * A_INSTR) * 1024u);
        const unsigned wbase_b = __builtin_amdgcn_readfirstlane(base + (unsigned)A_FLOATS * 4u + (unsigned)(wave * B_INSTR) * 1024u);
        if (!(NIC_TUNE(1) && in_loop)) {
#pragma unroll
            for (int q = 0; q < A_INSTR; ++q) dma16(ra, offA[q], wbase_a + q * 1024u);
        }
        if (!(NIC_TUNE(2) && in_loop)) {
#pragma unroll
            for (int q = 0; q < B_INSTR; ++q) dma16(rb, offB[q], wbase_b + q * 1024u);
        }
    };
    auto advance = [&]() {
#pragma unroll
        for (int q = 0; q < A_INSTR; ++q) offA[q] += BK * 4;
#pragma unroll
        for (int q = 0; q < B_INSTR; ++q) offB[q] += stepB;
    };

    f32x16 acc[MT][NT];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    // swizzled chunk positions of this lane's A rows: row = wm*MT*32 + i*32 + li -> ((row >> 1) & 7) == ((li >> 1) & 7)
    const int sw = (li >> 1) & 7;
    const int nk = (p.K + BK - 1) / BK;
    // epilogue geometry (needed here already: the dgrad epilogue's Hprev rows are fetched during the last k tiles)
    constexpr int TPR = BN / 4, RPI = NTHREADS / TPR, ITER = PASS_ROWS / RPI;
    static_assert(PASS_ROWS % RPI == 0, "pass rows must divide evenly over the threads");
    const int t = threadIdx.x;
    const int col = c0 + (t % TPR) * 4;
    // EPI_DGRAD multiplies the tile by act'(Hprev): read in the epilogue, those 256 KB per workgroup arrive as one burst from
    // every CU at once, on top of the write burst.  The kernel has ~80 free VGPRs, so the rows of the first pass are fetched
    // into registers during the last PFT k tiles (each batch completes under that tile's MFMAs, before its dma_wait), and
    // the rows of the second pass are fetched into the same registers as the first pass consumes them.
    constexpr int PFT = (ITER % 4 == 0) ? 4 : 2;
    static_assert(ITER % PFT == 0, "prefetch batches must divide the pass");
    // (the 7-row-tile wave holds 112 accumulators + 56 fragment registers: no room for the prefetch registers as well)
    constexpr bool PREFETCH_H = EPI == EPI_DGRAD && MT <= 4;
    float4 hq[PREFETCH_H ? ITER : 1];  // (dead in the forward instantiation)
    const bool pf_on = PREFETCH_H && p.Hprev != nullptr && p.act == NIC_ACT_ELU && nk >= PFT && !p.accumulate && !NIC_TUNE(8);
    auto load_h = [&](int pass, int it) {
        const int row = m0 + pass * PASS_ROWS + t / TPR + RPI * it;
        return (row < p.M && col < p.ncols) ? *reinterpret_cast<const float4*>(p.Hprev + (int64_t)row * p.ldb + col)
                                            : make_float4(0.f, 0.f, 0.f, 0.f);
    };

    auto ktile = [&](int kt) {
        const int cur = kt & 1;
        if (kt + 1 < nk) {  // stage cur^1 was last read in tile kt-1; every wave is past that barrier
            advance();
            issue(cur ^ 1);
        }
        const float* a_base = lds + cur * STAGE + (wm * MT * 32 + li) * BK;
        const float* b_base = lds + cur * STAGE + A_FLOATS + wn * NT * 32 + li;
#pragma unroll
        for (int g = 0; g < 2; ++g) {
            float a[MT][8];
#pragma unroll
            for (int i = 0; i < MT; ++i) {
                const float4 lo = *reinterpret_cast<const float4*>(a_base + i * 32 * BK + (((g * 4 + h * 2) ^ sw) << 2));
                const float4 hi = *reinterpret_cast<const float4*>(a_base + i * 32 * BK + (((g * 4 + h * 2 + 1) ^ sw) << 2));
                a[i][0] = lo.x; a[i][1] = lo.y; a[i][2] = lo.z; a[i][3] = lo.w;
                a[i][4] = hi.x; a[i][5] = hi.y; a[i][6] = hi.z; a[i][7] = hi.w;
            }
#pragma unroll
            for (int kk = 0; kk < 8; ++kk) {
                float b[NT];
#pragma unroll
                for (int j = 0; j < NT; ++j) b[j] = b_base[(g * 16 + h * 8 + kk) * BN + j * 32];
#pragma unroll
                for (int i = 0; i < MT; ++i)
#pragma unroll
                    for (int j = 0; j < NT; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i][kk], b[j], acc[i][j], 0, 0, 0);
            }
        }
        dma_wait();  // tile kt+1 has landed (this wave's share); the barrier publishes every wave's share
        if (!NIC_TUNE(4)) __syncthreads();
    };
    issue(0);
    dma_wait();
    __syncthreads();
    NIC_STAMP(1);
    in_loop = true;
#ifdef NIC_TUNING_BUILD
    // static priority for the younger half of the workgroup (cdna_hip_programming.md T5, static form)
    if (NIC_TUNE(32) && __builtin_amdgcn_readfirstlane(threadIdx.x) >= NTHREADS / 2) __builtin_amdgcn_s_setprio(1);
#endif
    const int nk_plain = pf_on ? nk - PFT : nk;
    for (int kt = 0; kt < nk_plain; ++kt) ktile(kt);
    if (NIC_TUNE(16)) NIC_STAMP(1);  // (tuning build: the "k loop" phase then covers the prefetch tiles alone)
    if constexpr (EPI == EPI_DGRAD) {
        if (pf_on) {
#pragma unroll
            for (int b = 0; b < PFT; ++b) {
#pragma unroll
                for (int q = 0; q < ITER / PFT; ++q) hq[PREFETCH_H ? b * (ITER / PFT) + q : 0] = load_h(0, b * (ITER / PFT) + q);
                ktile(nk_plain + b);
            }
        }
    }

    NIC_STAMP(2);
    // epilogue: stage the block tile through LDS and write whole rows
    float* cs = lds;
    // Production case first (whole tile inside the matrix; forward: bias + ELU, dgrad: prefetched Hprev): straight-line row
    // loop, no per-row guards or option branches, so hipcc hoists the bias loads and keeps exact s_waitcnt counts — the
    // refill loads and the stores of one row do not stall the next row.
    const bool full_tile = m0 + BM <= p.M && c0 + BN <= p.ncols;
    const bool fast_epi = full_tile && (EPI == EPI_DGRAD ? pf_on : (p.bias != nullptr && p.act == NIC_ACT_ELU));
#ifdef NIC_TUNING_BUILD
    if (EPI == EPI_BIAS_ACT && fast_epi && NIC_TUNE(64)) {
        // experiment: forward epilogue straight from the accumulators (no LDS staging, no barriers): one dword store per
        // accumulator register, 32 lanes = 128 contiguous bytes of a row, the wave's two halves four rows apart
        const int64_t base = (int64_t)(m0 + wm * MT * 32 + 4 * h) * p.ldb + c0 + wn * NT * 32 + li;
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int rl = i * 32 + (r & 3) + 8 * (r >> 2);
                const float bias = p.bias[m0 + wm * MT * 32 + 4 * h + rl];
#pragma unroll
                for (int j = 0; j < NT; ++j) p.C[base + (int64_t)rl * p.ldb + j * 32] = elu_f(acc[i][j][r] + bias);
            }
        NIC_STAMP(3);
        return;
    }
#endif
    if (fast_epi) {
#pragma unroll
        for (int pass = 0; pass < PASSES; ++pass) {
            if (PASSES == 1 || wm == pass) {
                const int wrow = (PASSES == 1) ? wm * MT * 32 : 0;
#pragma unroll
                for (int i = 0; i < MT; ++i)
#pragma unroll
                    for (int j = 0; j < NT; ++j)
#pragma unroll
                        for (int r = 0; r < 16; ++r)
                            cs[(wrow + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * h) * LDC + (wn * NT + j) * 32 + li] = acc[i][j][r];
            }
            __syncthreads();
            const int row0 = m0 + pass * PASS_ROWS + t / TPR;
            float bias_r[ITER];
            if (EPI == EPI_BIAS_ACT) {
#pragma unroll
                for (int it = 0; it < ITER; ++it) bias_r[it] = p.bias[row0 + RPI * it];
            }
            // 32-bit element offset, advanced row group by row group (M * ldb < 2^28 on this path): one address register
            int off = row0 * (int)p.ldb + col;
            const int off_step = RPI * (int)p.ldb, off_pass = PASS_ROWS * (int)p.ldb;
#pragma unroll
            for (int it = 0; it < ITER; ++it, off += off_step) {
                const int row_l = t / TPR + RPI * it;
                float4 y = *reinterpret_cast<const float4*>(cs + row_l * LDC + (t % TPR) * 4);
                if (EPI == EPI_BIAS_ACT) {
                    y.x = elu_f(y.x + bias_r[it]); y.y = elu_f(y.y + bias_r[it]);
                    y.z = elu_f(y.z + bias_r[it]); y.w = elu_f(y.w + bias_r[it]);
                } else {
                    const float4 hv = hq[PREFETCH_H ? it : 0];
                    y.x *= elu_grad_from_out(hv.x); y.y *= elu_grad_from_out(hv.y);
                    y.z *= elu_grad_from_out(hv.z); y.w *= elu_grad_from_out(hv.w);
                    if (pass + 1 < PASSES)  // next pass's row into the freed register
                        hq[PREFETCH_H ? it : 0] = *reinterpret_cast<const float4*>(p.Hprev + off + off_pass);
                }
                *reinterpret_cast<float4*>(p.C + off) = y;
                // keep the scheduler from hoisting all 16 staged rows (64 VGPRs on top of 128 accumulators + 64 Hprev
                // registers spills): rows are scheduled in groups of four
                if ((it & 3) == 3) __builtin_amdgcn_sched_barrier(0);
            }
            if (pass + 1 < PASSES) __syncthreads();
        }
        NIC_STAMP(3);
        return;
    }
#pragma unroll
    for (int pass = 0; pass < PASSES; ++pass) {
        if (PASSES == 1 || wm == pass) {
            const int wrow = (PASSES == 1) ? wm * MT * 32 : 0;
#pragma unroll
            for (int i = 0; i < MT; ++i)
#pragma unroll
                for (int j = 0; j < NT; ++j)
#pragma unroll
                    for (int r = 0; r < 16; ++r)
                        cs[(wrow + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * h) * LDC + (wn * NT + j) * 32 + li] = acc[i][j][r];
        }
        __syncthreads();
        float bias_g[ITER];   // (fetched together: one load - wait - store round trip per row otherwise)
#pragma unroll
        for (int it = 0; it < ITER; ++it) {
            const int row = m0 + pass * PASS_ROWS + t / TPR + RPI * it;
            bias_g[it] = (EPI == EPI_BIAS_ACT && p.bias) ? p.bias[row < p.M ? row : 0] : 0.f;
        }
#pragma unroll
        for (int it = 0; it < ITER; ++it) {
            const int row_l = t / TPR + RPI * it;
            const int row = m0 + pass * PASS_ROWS + row_l;
            if (row >= p.M || col >= p.ncols) continue;
            float4 y = *reinterpret_cast<const float4*>(cs + row_l * LDC + (t % TPR) * 4);
            const int64_t off = (int64_t)row * p.ldb + col;
            if (EPI == EPI_BIAS_ACT) {
                const float bias = bias_g[it];
                y.x += bias; y.y += bias; y.z += bias; y.w += bias;
                if (p.act == NIC_ACT_ELU) { y.x = elu_f(y.x); y.y = elu_f(y.y); y.z = elu_f(y.z); y.w = elu_f(y.w); }
            } else {
                if (p.Hprev && p.act == NIC_ACT_ELU) {
                    const float4 hv = pf_on ? hq[PREFETCH_H ? it : 0] : *reinterpret_cast<const float4*>(p.Hprev + off);
                    y.x *= elu_grad_from_out(hv.x); y.y *= elu_grad_from_out(hv.y);
                    y.z *= elu_grad_from_out(hv.z); y.w *= elu_grad_from_out(hv.w);
                    if (pf_on && pass + 1 < PASSES) hq[PREFETCH_H ? it : 0] = load_h(pass + 1, it);  // next pass's row into the freed register
                }
                if (p.accumulate) {
                    const float4 o = *reinterpret_cast<const float4*>(p.C + off);
                    y.x += o.x; y.y += o.y; y.z += o.z; y.w += o.w;
                }
            }
            *reinterpret_cast<float4*>(p.C + off) = y;
        }
        if (pass + 1 < PASSES) __syncthreads();
    }
#endif
}

// ---------------------------------------------------------------------------------------------------------------
// wx kernel, streamed form for SMALL launches (round 4): the reference's shipped batch of 1,024 scenarios, the thin logits /
// first-layer-gradient GEMMs at every batch size.  A launch with a few hundred 32 x 32 output tiles cannot fill the chip with
// workgroup tiles, and a lone workgroup's LDS pipeline pays ~0.45 us of copy round trip + barrier per 32-deep k tile that
// nothing overlaps (16 k tiles: 13-25 us for 0.5 GFLOP).  Here ONE WAVEFRONT owns a 32 x (32 NT) output tile and reads its
// operands straight from L2 into registers - no LDS tile, no barrier in the k loop: per 16-deep k group a lane fetches its 8
// A values as two 16-byte loads (row m0 + lane, k contiguous) and its 8 NT B values as dword loads (rows of X: 128 contiguous
// bytes per half wave), D = 4 groups ahead of the MFMAs that consume them (counted vmcnt, no waits on the critical path).
// KS wavefronts of a workgroup split the contraction (K / KS each) and add their accumulators through LDS once, so even a
// 17-row logits layer at 1,024 scenarios is 32 tiles x 4 = 128 wavefronts with 8 k groups each instead of one 16-tile chain.
// Operand traffic is tiles x K x 32 (1 + NT) x 4 B from L2 (weights and the activations of a small batch are L2-resident):
// only worth it while that stays below ~100 MB - pick_wx_stream (wx_plan.h).
// Same k order as the LDS-DMA kernel within a group (lanes 0-31: k = kk, lanes 32-63: k = 8 + kk).
// ---------------------------------------------------------------------------------------------------------------
template <int NT, int KS, int EPI, bool MODELS = false, bool MASKED = false>
__global__ __launch_bounds__(64 * KS) void gemm_wx_stream_kernel(WxArgs<MASKED> p) {
    if constexpr (MODELS) {
        if constexpr (MASKED) {
            if (model_stopped(p)) return;
        }
        advance_models(p);
    }
    constexpr int D = 4;
    __shared__ float red[(KS > 1 ? KS - 1 : 1) * NT * 16 * 64];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int li = lane & 31, h = lane >> 5;
    const int tiles_m = (p.M + 31) / 32;
    const int tile = xcd_swizzle(blockIdx.x, gridDim.x);   // the row tiles of one column panel run on one XCD (shared L2)
    const int m0 = (tile % tiles_m) * 32, c0 = (tile / tiles_m) * (32 * NT);
    const __amdgpu_buffer_rsrc_t rA = make_rsrc(p.A, (int64_t)p.M * p.lda), rB = make_rsrc(p.Bm, (int64_t)p.K * p.ldb);
    // this wavefront's k groups: [g_lo, g_lo + per), per a multiple of D; groups past K read B rows beyond the descriptor (zeros)
    const int ng_all = (p.K + 15) / 16;
    const int per = ((ng_all + KS - 1) / KS + D - 1) / D * D, nblk = per / D;
    const int g_lo = wave * per;
    const int ldb4 = (int)p.ldb * 4;
    int offA = (int)((((int64_t)m0 + li) * p.lda + g_lo * 16 + h * 8) * 4);
    int offB = (int)((((int64_t)g_lo * 16 + h * 8) * p.ldb + c0 + li) * 4);

    f32x16 acc[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
    float a[D][8], b[D][NT][8];
    auto load = [&](int d) {
        const float4 lo = buf_load4(rA, offA), hi = buf_load4(rA, offA + 16);
        a[d][0] = lo.x; a[d][1] = lo.y; a[d][2] = lo.z; a[d][3] = lo.w;
        a[d][4] = hi.x; a[d][5] = hi.y; a[d][6] = hi.z; a[d][7] = hi.w;
#pragma unroll
        for (int kk = 0; kk < 8; ++kk)
#pragma unroll
            for (int j = 0; j < NT; ++j)
                b[d][j][kk] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rB, offB + j * 128, kk * ldb4, 0));
        offA += 64;
        offB += 16 * ldb4;
    };
    auto compute = [&](int d) {
#pragma unroll
        for (int kk = 0; kk < 8; ++kk)
#pragma unroll
            for (int j = 0; j < NT; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[d][kk], b[d][j][kk], acc[j], 0, 0, 0);
    };
#pragma unroll
    for (int d = 0; d < D; ++d) load(d);
    for (int blk = 0; blk + 1 < nblk; ++blk) {
#pragma unroll
        for (int d = 0; d < D; ++d) {
            compute(d);
            load(d);
        }
    }
    // the epilogue's own operands are fetched under the last block's MFMAs (wave 0 writes the tile)
    const int row_base = m0 + 4 * h;   // accumulator register r holds row row_base + (r & 3) + 8 (r >> 2), column c0 + 32 j + li
    float aux[16];   // forward: bias[row]; dgrad: act'(Hprev) of tile column j = 0 (further columns are read in the epilogue)
    const bool use_h = EPI == EPI_DGRAD && p.Hprev != nullptr && p.act == NIC_ACT_ELU;
    if (wave == 0) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = row_base + (r & 3) + 8 * (r >> 2);
            const bool ok = row < p.M && c0 + li < p.ncols;
            if (EPI == EPI_BIAS_ACT) aux[r] = (p.bias != nullptr && row < p.M) ? p.bias[row] : 0.f;
            else aux[r] = (use_h && ok) ? p.Hprev[(int64_t)row * p.ldb + c0 + li] : 1.f;
        }
    }
#pragma unroll
    for (int d = 0; d < D; ++d) compute(d);

    if constexpr (KS > 1) {
        if (wave > 0) {
#pragma unroll
            for (int j = 0; j < NT; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) red[(((wave - 1) * NT + j) * 16 + r) * 64 + lane] = acc[j][r];
        }
        __syncthreads();
        if (wave > 0) return;
#pragma unroll
        for (int w = 0; w < KS - 1; ++w)
#pragma unroll
            for (int j = 0; j < NT; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[j][r] += red[((w * NT + j) * 16 + r) * 64 + lane];
    }
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        const int col = c0 + j * 32 + li;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = row_base + (r & 3) + 8 * (r >> 2);
            if (row >= p.M || col >= p.ncols) continue;
            const int64_t off = (int64_t)row * p.ldb + col;
            float y = acc[j][r];
            if (EPI == EPI_BIAS_ACT) {
                y += aux[r];
                if (p.act == NIC_ACT_ELU) y = elu_f(y);
            } else {
                if (use_h) y *= elu_grad_from_out(j == 0 ? aux[r] : p.Hprev[off]);
                if (p.accumulate) y += p.C[off];
            }
            p.C[off] = y;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// wgrad kernel: slab[split][n][k] += sum_{b in split} dY[n][b] * X[k][b]   (k == K: bias column, X row of ones)
// ---------------------------------------------------------------------------------------------------------------
struct WgParams {
    const float* dY;  // [N][ldb]
    const float* X;   // [K][ldb]
    float* slab;      // [n_splits][N][lds]
    int64_t lds_, ldb;
    int N, K, nB, chunk;  // chunk = scenarios per split (multiple of 32)
    int swz;              // XCD-aware tile order (DMA kernel)
    // periods (DMA kernel): the contraction runs over n_periods operand pairs dY + t * pstride_dy, X + t * pstride_x (elements)
    // with the same scenario split in each — one launch for the whole backward sweep of a rollout
    int n_periods;
    int64_t pstride_dy, pstride_x;
    // the register accumulators are added to the slab and cleared every `flush_periods` periods: an fp32 sum of 10^5
    // terms in one register drifts to ~5e-5 relative (measured against the fp32 CPU reference at T = 100 x 1,024 scenarios
    // per split); 8k-term partial sums keep the weight gradients at the per-period accuracy
    int flush_periods;
    // round 4: the slab slots are (period group, scenario split) pairs - slot = group * scen_splits + scenario split; a group
    // contracts periods [group * periods_per_group, ...) only.  Few scenarios x many periods (the reference's shipped batch of
    // 1,024, an 8-GPU shard of 8,192) then still gives every CU a workgroup.  scen_splits = 0: one group (all slots are
    // scenario splits).
    int scen_splits, periods_per_group;
    // model form (MODELS instantiations, grid y = model): floats between two models' dY, X and slab
    int64_t m_dy, m_x, m_slab;
};
struct WgModelParams : WgParams { const int32_t* active; };   // (the MASKED instantiations': with the active-model mask, as WxModelParams)
template <bool MASKED> using WgArgs = std::conditional_t<MASKED, WgModelParams, WgParams>;
__device__ __forceinline__ void advance_models(WgParams& p) {
    p.dY += nic::linear_model_offset(blockIdx.y, p.m_dy);
    p.X += nic::linear_model_offset(blockIdx.y, p.m_x);
    p.slab += nic::linear_model_offset(blockIdx.y, p.m_slab);
}

template <int WAVES_M, int WAVES_N, int MT, int NT, int FAST, bool MODELS = false, bool MASKED = false>
__global__ __launch_bounds__(kThreads) void gemm_wgrad_kernel(WgArgs<MASKED> p) {
    if constexpr (MODELS) {
        if constexpr (MASKED) {
            if (model_stopped(p)) return;
        }
        advance_models(p);
    }
    constexpr int BM = WAVES_M * MT * 32;
    constexpr int BN = WAVES_N * NT * 32;
    constexpr int STAGE = (BM + BN) * LDA_S;
    __shared__ __attribute__((aligned(16))) float lds[2 * STAGE];

    // 1-D grid, tile index fastest: the tiles of one scenario chunk (split) are contiguous logical ids -> one XCD
    const int tiles_k = (p.K + 1 + BN - 1) / BN, tiles_n = (p.N + BM - 1) / BM;
    const int lid = blockIdx.x;  // (an XCD remap of this id measured 15 % SLOWER here: keep dispatch order)
    const int k0 = (lid % tiles_k) * BN;                  // output cols  (features of X, plus the bias column K)
    const int n0 = ((lid / tiles_k) % tiles_n) * BM;      // output rows  (features of dY)
    const int split = lid / (tiles_k * tiles_n);
    // slab slot = (period group, scenario split) when scen_splits > 0 (see WgParams): this workgroup's periods
    const int ssplit = p.scen_splits > 0 ? split % p.scen_splits : split;
    const int p_first = p.scen_splits > 0 ? (split / p.scen_splits) * p.periods_per_group : 0;
    const int p_end = p.scen_splits > 0 ? min(p_first + p.periods_per_group, p.n_periods) : p.n_periods;
    const int b_begin = ssplit * p.chunk;
    const int b_end = min(b_begin + p.chunk, p.nB);

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wm = wave / WAVES_N, wn = wave % WAVES_N;
    const int li = lane & 31, h = lane >> 5;
    float* slab = p.slab + (int64_t)split * p.N * p.lds_;

    // accumulators start from the slab (the running sum over the periods of the rollout)
    f32x16 acc[MT][NT];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = n0 + (wm * MT + i) * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
                const int col = k0 + (wn * NT + j) * 32 + li;
                acc[i][j][r] = (row < p.N && col <= p.K) ? slab[(int64_t)row * p.lds_ + col] : 0.f;
            }

    // periods: the accumulators persist over n_periods operand pairs (one slab read-modify-write per launch)
    for (int period = p_first; period < p_end && b_begin < b_end; ++period) {
        const float* dYp = p.dY + period * p.pstride_dy;
        const float* Xp = p.X + period * p.pstride_x;
        if (period > p_first) __syncthreads();  // the previous period's last tile has been read by every wave
        const bool vec = (p.ldb % 4 == 0) && ((reinterpret_cast<uintptr_t>(dYp) & 15) == 0) &&
                         ((reinterpret_cast<uintptr_t>(Xp) & 15) == 0);
        KTile<BM> ta;
        KTile<BN> tb;
        KTileBuf<BM> fa;
        KTileBuf<BN> fb;
        __amdgpu_buffer_rsrc_t ra, rb;
        const int nt = (b_end - b_begin + BK - 1) / BK;
        if constexpr (FAST) {
            ra = make_rsrc(dYp, (int64_t)p.N * p.ldb);
            rb = make_rsrc(Xp, (int64_t)p.K * p.ldb);
            fa.init(p.ldb, n0, b_begin);
            fb.init(p.ldb, k0, b_begin);
            fa.load(ra);
            fb.load(rb);
            fa.mask_cols(b_begin, b_end, n0, -1);
            fb.mask_cols(b_begin, b_end, k0, p.K);
            fa.store(lds);
            fb.store(lds + BM * LDA_S);
        } else {
            ta.load(dYp, p.ldb, n0, p.N, b_begin, b_end, vec);
            tb.load(Xp, p.ldb, k0, p.K, b_begin, b_end, vec, p.K, b_end);
            ta.store(lds);
            tb.store(lds + BM * LDA_S);
        }
        __syncthreads();
        for (int t = 0; t < nt; ++t) {
            const int cur = t & 1;
            if (t + 1 < nt) {
                if constexpr (FAST) {
                    fa.advance();
                    fb.advance();
                    fa.load(ra);
                    fb.load(rb);
                } else {
                    ta.load(dYp, p.ldb, n0, p.N, b_begin + (t + 1) * BK, b_end, vec);
                    tb.load(Xp, p.ldb, k0, p.K, b_begin + (t + 1) * BK, b_end, vec, p.K, b_end);
                }
            }
            const float* a_base = lds + cur * STAGE + (wm * MT * 32 + li) * LDA_S;
            const float* b_base = lds + cur * STAGE + (BM + wn * NT * 32 + li) * LDA_S;
#pragma unroll
            for (int g = 0; g < 2; ++g) {
                float a[MT][8], b[NT][8];
#pragma unroll
                for (int i = 0; i < MT; ++i) read_frag8(a_base + i * 32 * LDA_S, g, h, a[i]);
#pragma unroll
                for (int j = 0; j < NT; ++j) read_frag8(b_base + j * 32 * LDA_S, g, h, b[j]);
#pragma unroll
                for (int kk = 0; kk < 8; ++kk)
#pragma unroll
                    for (int i = 0; i < MT; ++i)
#pragma unroll
                        for (int j = 0; j < NT; ++j)
                            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i][kk], b[j][kk], acc[i][j], 0, 0, 0);
            }
            if (t + 1 < nt) {
                if constexpr (FAST) {
                    fa.mask_cols(b_begin + (t + 1) * BK, b_end, n0, -1);
                    fb.mask_cols(b_begin + (t + 1) * BK, b_end, k0, p.K);
                    fa.store(lds + (cur ^ 1) * STAGE);
                    fb.store(lds + (cur ^ 1) * STAGE + BM * LDA_S);
                } else {
                    ta.store(lds + (cur ^ 1) * STAGE);
                    tb.store(lds + (cur ^ 1) * STAGE + BM * LDA_S);
                }
            }
            __syncthreads();
        }
    }

#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = n0 + (wm * MT + i) * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
                const int col = k0 + (wn * NT + j) * 32 + li;
                if (row < p.N && col <= p.K) slab[(int64_t)row * p.lds_ + col] = acc[i][j][r];
            }
}

// ---------------------------------------------------------------------------------------------------------------
// wgrad kernel, LDS-DMA form: both operands are row tiles with the contraction index (scenario) contiguous, so both use
// the swizzled 1-KiB DMA of the wx kernel's A tile.  Output tile BM x BN of dW for one scenario chunk (split); the tile is
// ADDED to the split's slab through the LDS-staged epilogue (whole-row float4 read-add-write).  The bias gradient needs
// no virtual row of ones here: the waves of the first column tile sum the dY fragments they read anyway.
// Requires n_scenarios % 32 == 0 (no partial k tiles) — the launcher falls back to gemm_wgrad_kernel otherwise.
// ---------------------------------------------------------------------------------------------------------------
// SKIP_ROWS: row tiles of a wave that lie entirely past N are not computed (N = 195 in a 256-row tile: the wave rows hold 4 and 3
// of the 7 row tiles with rows, and the two wavefronts of a SIMD are (wm = 0, wn) and (wm = 1, wn)).
template <int WAVES_M, int WAVES_N, int MT, int NT, bool SKIP_ROWS = false>
__global__ __launch_bounds__(64 * WAVES_M * WAVES_N) void gemm_wgrad_dma_kernel(WgParams p) {
#if defined(__HIP_DEVICE_COMPILE__)
    constexpr int NW = WAVES_M * WAVES_N, NTHREADS = 64 * NW;
    constexpr int BM = WAVES_M * MT * 32;
    constexpr int BN = WAVES_N * NT * 32;
    constexpr int A_FLOATS = BM * BK, B_FLOATS = BN * BK, STAGE = A_FLOATS + B_FLOATS;
    constexpr int LDC = BN + 4;
    constexpr int PASSES = (BM * LDC * 4 <= 72 * 1024) ? 1 : WAVES_M;
    constexpr int PASS_ROWS = BM / PASSES;
    constexpr int LDS_FLOATS = (2 * STAGE > PASS_ROWS * LDC) ? 2 * STAGE : PASS_ROWS * LDC;
    __shared__ __attribute__((aligned(16))) float lds[LDS_FLOATS];
    typedef __attribute__((address_space(3))) void* lds_ptr_t;

    const int tiles_k = (p.K + BN - 1) / BN, tiles_n = (p.N + BM - 1) / BM;
    // the output tiles of one scenario chunk read the same dY / X rows: keep them on one XCD (shared L2)
    const int lid = p.swz ? xcd_swizzle(blockIdx.x, gridDim.x) : (int)blockIdx.x;
    const int k0 = (lid % tiles_k) * BN;              // output cols (features of X)
    const int n0 = ((lid / tiles_k) % tiles_n) * BM;  // output rows (features of dY)
    const int split = lid / (tiles_k * tiles_n);
    const int ssplit = p.scen_splits > 0 ? split % p.scen_splits : split;   // scenario split / period group of this slab slot
    const int pgroup = p.scen_splits > 0 ? split / p.scen_splits : 0;
    const int p_first = pgroup * p.periods_per_group;
    const int n_per = p.scen_splits > 0 ? min(p.periods_per_group, p.n_periods - p_first) : p.n_periods;
    const int b_begin = ssplit * p.chunk;
    const int b_end = min(b_begin + p.chunk, p.nB);
    const int nt = (b_end - b_begin) / BK;            // whole tiles only (nB % 32 == 0)
    if (nt <= 0 || n_per <= 0) return;

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wm = wave / WAVES_N, wn = wave % WAVES_N;
    const int li = lane & 31, h = lane >> 5;
    float* slab = p.slab + (int64_t)split * p.N * p.lds_;

    u32x4 ra = make_desc(p.dY + p_first * p.pstride_dy, (int64_t)p.N * p.ldb);
    u32x4 rb = make_desc(p.X + p_first * p.pstride_x, (int64_t)p.K * p.ldb);
    const unsigned lds0 = (unsigned)(uintptr_t)(lds_ptr_t)lds;
    constexpr int A_INSTR = BM / 8 / NW, B_INSTR = BN / 8 / NW;
    int offA[A_INSTR], offB[B_INSTR];
#pragma unroll
    for (int q = 0; q < A_INSTR; ++q) {
        const int row = (wave * A_INSTR + q) * 8 + (lane >> 3);
        const int chunk = (lane & 7) ^ ((row >> 1) & 7);
        offA[q] = (int)((((int64_t)n0 + row) * p.ldb + b_begin + chunk * 4) * 4);
    }
#pragma unroll
    for (int q = 0; q < B_INSTR; ++q) {
        const int row = (wave * B_INSTR + q) * 8 + (lane >> 3);
        const int chunk = (lane & 7) ^ ((row >> 1) & 7);
        offB[q] = (int)((((int64_t)k0 + row) * p.ldb + b_begin + chunk * 4) * 4);
    }
    auto issue = [&](int stage) {
        const unsigned base = __builtin_amdgcn_readfirstlane(lds0 + (unsigned)(stage * STAGE) * 4u);
        const unsigned wbase_a = __builtin_amdgcn_readfirstlane(base + (unsigned)(wave * A_INSTR) * 1024u);
        const unsigned wbase_b = __builtin_amdgcn_readfirstlane(base + (unsigned)A_FLOATS * 4u + (unsigned)(wave * B_INSTR) * 1024u);
#pragma unroll
        for (int q = 0; q < A_INSTR; ++q) dma16(ra, offA[q], wbase_a + q * 1024u);
#pragma unroll
        for (int q = 0; q < B_INSTR; ++q) dma16(rb, offB[q], wbase_b + q * 1024u);
    };
    auto advance = [&]() {
#pragma unroll
        for (int q = 0; q < A_INSTR; ++q) offA[q] += BK * 4;
#pragma unroll
        for (int q = 0; q < B_INSTR; ++q) offB[q] += BK * 4;
    };

    f32x16 acc[MT][NT];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    float rowsum[MT];
#pragma unroll
    for (int i = 0; i < MT; ++i) rowsum[i] = 0.f;
    const bool bias_owner = (k0 == 0) && (wn == 0);  // these waves also produce the bias-gradient column
    const int rows_left = p.N - n0 - wm * MT * 32;
    const bool full_rows = rows_left > (MT - 1) * 32, some_rows = rows_left > 0;

    const int sw = (li >> 1) & 7;
    issue(0);
    dma_wait();
    __syncthreads();
    // flat sequence of (period, k tile): the copy of the next tile crosses period boundaries by moving the two buffer
    // descriptors to the next period's operands and rewinding the offsets, so the pipeline never drains
    const int total = nt * n_per;
    const int group = nt * (p.flush_periods > 0 ? p.flush_periods : n_per);  // tiles between two slab updates
    int t_in = 0, period = p_first;
    auto next_tile = [&]() {  // moves descriptors / offsets to tile t+1 (possibly the first tile of the next period)
        if (++t_in == nt) {
            t_in = 0;
            ++period;
            ra = make_desc(p.dY + period * p.pstride_dy, (int64_t)p.N * p.ldb);
            rb = make_desc(p.X + period * p.pstride_x, (int64_t)p.K * p.ldb);
#pragma unroll
            for (int q = 0; q < A_INSTR; ++q) offA[q] -= (nt - 1) * BK * 4;
#pragma unroll
            for (int q = 0; q < B_INSTR; ++q) offB[q] -= (nt - 1) * BK * 4;
        } else {
            advance();
        }
    };
    // threads per output row, rounded up to a power of two (BN = 448: 112 -> 128, the last 16 threads of a row group idle)
    constexpr int TPR_USED = BN / 4;
    constexpr int TPR = TPR_USED <= 16 ? 16 : TPR_USED <= 32 ? 32 : TPR_USED <= 64 ? 64 : 128;
    constexpr int RPI = NTHREADS / TPR, ITER = PASS_ROWS / RPI;
    static_assert(TPR_USED <= 128 && PASS_ROWS % RPI == 0, "epilogue row groups must tile the pass");
    const int tt = threadIdx.x;
    const bool col_thread = (tt % TPR) < TPR_USED;
    const int col = k0 + (tt % TPR) * 4;
    float* cs = lds;
    auto flush = [&]() {  // slab += accumulators (all waves; uses the whole staging area, so no copy may be in flight)
    // bias gradient: lanes l and l+32 hold the two k halves of row (wm*MT + i)*32 + li
        if (bias_owner) {
#pragma unroll
            for (int i = 0; i < MT; ++i) {
                const float s = rowsum[i] + __shfl_xor(rowsum[i], 32);
                const int row = n0 + (wm * MT + i) * 32 + li;
                if (h == 0 && row < p.N) slab[(int64_t)row * p.lds_ + p.K] += s;
            }
        }

        // slab += tile, staged through LDS (whole-row float4 read-add-write)
#pragma unroll
        for (int pass = 0; pass < PASSES; ++pass) {
            if (PASSES == 1 || wm == pass) {
                const int wrow = (PASSES == 1) ? wm * MT * 32 : 0;
#pragma unroll
                for (int i = 0; i < MT; ++i)
#pragma unroll
                    for (int j = 0; j < NT; ++j)
#pragma unroll
                        for (int r = 0; r < 16; ++r)
                            cs[(wrow + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * h) * LDC + (wn * NT + j) * 32 + li] = acc[i][j][r];
            }
            __syncthreads();
#pragma unroll
            for (int it = 0; it < ITER; ++it) {
                const int row_l = tt / TPR + RPI * it;
                const int row = n0 + pass * PASS_ROWS + row_l;
                if (row >= p.N || col >= p.K || !col_thread) continue;
                const float4 y = *reinterpret_cast<const float4*>(cs + row_l * LDC + (tt % TPR) * 4);
                float* dst = slab + (int64_t)row * p.lds_ + col;
                if (col + 3 < p.K && (p.lds_ & 3) == 0) {
                    float4 o = *reinterpret_cast<const float4*>(dst);
                    o.x += y.x; o.y += y.y; o.z += y.z; o.w += y.w;
                    *reinterpret_cast<float4*>(dst) = o;
                } else {
                    dst[0] += y.x;
                    if (col + 1 < p.K) dst[1] += y.y;
                    if (col + 2 < p.K) dst[2] += y.z;
                    if (col + 3 < p.K) dst[3] += y.w;
                }
            }
            if (pass + 1 < PASSES) __syncthreads();
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < MT; ++i) {
            rowsum[i] = 0.f;
#pragma unroll
            for (int j = 0; j < NT; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
        }
    };
    for (int t = 0; t < total; ++t) {
        const int cur = t & 1;
        const bool boundary = (t + 1) % group == 0 || t + 1 == total;  // this tile ends an accumulation group
        if (!boundary) {
            next_tile();
            issue(cur ^ 1);
        }
        const float* a_base = lds + cur * STAGE + (wm * MT * 32 + li) * BK;
        const float* b_base = lds + cur * STAGE + A_FLOATS + (wn * NT * 32 + li) * BK;
        auto body = [&](auto mtv_c) {
            constexpr int MTV = decltype(mtv_c)::value;
#pragma unroll
            for (int g = 0; g < 2; ++g) {
                float a[MTV][8], b[NT][8];
#pragma unroll
                for (int i = 0; i < MTV; ++i) {
                    const float4 lo = *reinterpret_cast<const float4*>(a_base + i * 32 * BK + (((g * 4 + h * 2) ^ sw) << 2));
                    const float4 hi = *reinterpret_cast<const float4*>(a_base + i * 32 * BK + (((g * 4 + h * 2 + 1) ^ sw) << 2));
                    a[i][0] = lo.x; a[i][1] = lo.y; a[i][2] = lo.z; a[i][3] = lo.w;
                    a[i][4] = hi.x; a[i][5] = hi.y; a[i][6] = hi.z; a[i][7] = hi.w;
                }
#pragma unroll
                for (int j = 0; j < NT; ++j) {
                    const float4 lo = *reinterpret_cast<const float4*>(b_base + j * 32 * BK + (((g * 4 + h * 2) ^ sw) << 2));
                    const float4 hi = *reinterpret_cast<const float4*>(b_base + j * 32 * BK + (((g * 4 + h * 2 + 1) ^ sw) << 2));
                    b[j][0] = lo.x; b[j][1] = lo.y; b[j][2] = lo.z; b[j][3] = lo.w;
                    b[j][4] = hi.x; b[j][5] = hi.y; b[j][6] = hi.z; b[j][7] = hi.w;
                }
                if (bias_owner) {
#pragma unroll
                    for (int i = 0; i < MTV; ++i)
#pragma unroll
                        for (int kk = 0; kk < 8; ++kk) rowsum[i] += a[i][kk];
                }
#pragma unroll
                for (int kk = 0; kk < 8; ++kk)
#pragma unroll
                    for (int i = 0; i < MTV; ++i)
#pragma unroll
                        for (int j = 0; j < NT; ++j)
                            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i][kk], b[j][kk], acc[i][j], 0, 0, 0);
            }
        };
        if constexpr (SKIP_ROWS && MT >= 2) {
            if (full_rows) body(std::integral_constant<int, MT>{});
            else if (some_rows) body(std::integral_constant<int, MT - 1>{});
        } else {
            body(std::integral_constant<int, MT>{});
        }
        dma_wait();
        __syncthreads();
        if (boundary) {
            flush();
            if (t + 1 < total) {  // re-prime the pipeline after the slab update
                next_tile();
                issue(cur ^ 1);
                dma_wait();
                __syncthreads();
            }
        }
    }
#endif
}

// ---------------------------------------------------------------------------------------------------------------
// wgrad for the SMALL layers (N <= 32, K <= 32; the whole-horizon rollout of the 32-wide policies contracts over
// T*ldb ~ millions of columns): one 32 x 32 accumulator per WAVE over the wave's own column range, four independent
// waves per workgroup (wave-private LDS tiles, no workgroup barrier).  HBM-bound by construction: every dY / X element is
// read exactly once (8 KiB per 16 MFMAs).  slab split index = global wave id; bias column from the dY fragment sums.
// ---------------------------------------------------------------------------------------------------------------
// KC = 32-column chunks of the output (K <= 32 KC input features of X): one accumulator and one wave-private B tile each
template <int KC, bool MODELS = false, bool MASKED = false>
__global__ __launch_bounds__(kThreads) void wgrad_small_kernel(WgArgs<MASKED> p, int n_splits) {
    if constexpr (MODELS) {
        if constexpr (MASKED) {
            if (model_stopped(p)) return;
        }
        advance_models(p);
    }
    __shared__ __attribute__((aligned(16))) float lds[4 * (1 + KC) * 32 * LDA_S];  // per wave: A tile then KC B tiles, [32][36]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int li = lane & 31, h = lane >> 5;
    const int split = blockIdx.x * 4 + wave;
    if (split >= n_splits) return;  // (tiles are wave-private: no workgroup barrier below)
    const int b_begin = split * p.chunk;
    const int b_end = min(b_begin + p.chunk, p.nB);
    float* As = lds + wave * ((1 + KC) * 32 * LDA_S);
    float* Bs = As + 32 * LDA_S;
    const __amdgpu_buffer_rsrc_t ra = make_rsrc(p.dY, (int64_t)p.N * p.ldb);  // rows >= N / K read as zeros
    const __amdgpu_buffer_rsrc_t rb = make_rsrc(p.X, (int64_t)p.K * p.ldb);
    // tile = 32 rows x 32 columns; lane l moves rows (l >> 3) + 8 q, columns (l & 7) * 4 .. +3
    int off[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) off[q] = (int)((((int64_t)(lane >> 3) + 8 * q) * p.ldb + b_begin + (lane & 7) * 4) * 4);
    const int chunk_step = (int)(32 * p.ldb * 4);  // byte offset between two 32-row chunks of X

    f32x16 acc[KC];
#pragma unroll
    for (int c = 0; c < KC; ++c)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[c][r] = 0.f;
    float rowsum = 0.f;
    float4 va[4], vb[KC][4];
    const int nt = (b_end - b_begin + BK - 1) / BK;
    if (nt > 0) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            va[q] = buf_load4(ra, off[q]);
#pragma unroll
            for (int c = 0; c < KC; ++c) vb[c][q] = buf_load4(rb, off[q] + c * chunk_step);
        }
    }
    for (int t = 0; t < nt; ++t) {
        // columns at or past b_end contribute nothing (only the last tile of the last split can be partial)
        const int cc = b_begin + t * BK + (lane & 7) * 4;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            float4 x = va[q];
            const bool tail = cc + 3 >= b_end;
            if (tail) {
                if (cc + 0 >= b_end) x.x = 0.f;
                if (cc + 1 >= b_end) x.y = 0.f;
                if (cc + 2 >= b_end) x.z = 0.f;
                if (cc + 3 >= b_end) x.w = 0.f;
            }
            *reinterpret_cast<float4*>(As + ((lane >> 3) + 8 * q) * LDA_S + (lane & 7) * 4) = x;
#pragma unroll
            for (int c = 0; c < KC; ++c) {
                float4 y = vb[c][q];
                if (tail) {
                    if (cc + 0 >= b_end) y.x = 0.f;
                    if (cc + 1 >= b_end) y.y = 0.f;
                    if (cc + 2 >= b_end) y.z = 0.f;
                    if (cc + 3 >= b_end) y.w = 0.f;
                }
                *reinterpret_cast<float4*>(Bs + c * 32 * LDA_S + ((lane >> 3) + 8 * q) * LDA_S + (lane & 7) * 4) = y;
            }
        }
        if (t + 1 < nt) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                off[q] += BK * 4;
                va[q] = buf_load4(ra, off[q]);
#pragma unroll
                for (int c = 0; c < KC; ++c) vb[c][q] = buf_load4(rb, off[q] + c * chunk_step);
            }
        }
        __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0): this wave's LDS writes have landed (tiles are wave-private)
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int g = 0; g < 2; ++g) {
            float a[8];
            read_frag8(As + li * LDA_S, g, h, a);
#pragma unroll
            for (int kk = 0; kk < 8; ++kk) rowsum += a[kk];
#pragma unroll
            for (int c = 0; c < KC; ++c) {
                float b[8];
                read_frag8(Bs + c * 32 * LDA_S + li * LDA_S, g, h, b);
#pragma unroll
                for (int kk = 0; kk < 8; ++kk) acc[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[kk], b[kk], acc[c], 0, 0, 0);
            }
        }
        __builtin_amdgcn_wave_barrier();  // fragment reads done before the next tile overwrites the LDS tiles
    }
    float* slab = p.slab + (int64_t)split * p.N * p.lds_;
#pragma unroll
    for (int c = 0; c < KC; ++c)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = (r & 3) + 8 * (r >> 2) + 4 * h;
            const int col = c * 32 + li;
            if (row < p.N && col < p.K) slab[(int64_t)row * p.lds_ + col] += acc[c][r];
        }
    const float s = rowsum + __shfl_xor(rowsum, 32);
    if (h == 0 && li < p.N) slab[(int64_t)li * p.lds_ + p.K] += s;
}

// floats between two models' slab, dW and db (the MODELS instantiations of the two reduce kernels, grid y = model)
struct ReduceModels { int64_t slab, dW, db; };
struct ReduceModelStrides : ReduceModels { const int32_t* active; };   // (the MASKED instantiations': with the active-model mask)
template <bool MASKED> using ReduceArgs = std::conditional_t<MASKED, ReduceModelStrides, ReduceModels>;

template <bool MODELS = false, bool MASKED = false>
__global__ void wgrad_reduce_kernel(const float* __restrict__ slab, int64_t lds_, int n_splits, float* __restrict__ dW,
                                    int64_t lddw, float* __restrict__ db, int N, int K, float scale, ReduceArgs<MASKED> m) {
    if constexpr (MODELS) {
        if constexpr (MASKED) {
            if (model_stopped(m)) return;
        }
        slab += nic::linear_model_offset(blockIdx.y, m.slab);
        dW += nic::linear_model_offset(blockIdx.y, m.dW);
        if (db) db += nic::linear_model_offset(blockIdx.y, m.db);
    }
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t total = (int64_t)N * (K + 1);
    if (idx >= total) return;
    const int n = (int)(idx / (K + 1)), k = (int)(idx % (K + 1));
    float s = 0.f;
    for (int sp = 0; sp < n_splits; ++sp) s += slab[((int64_t)sp * N + n) * lds_ + k];
    s *= scale;
    if (k < K) dW[(int64_t)n * lddw + k] = s;
    else if (db) db[n] = s;
}

// many splits, few outputs (the small layers): one wavefront per output element, lanes stride over the splits
template <bool MODELS = false, bool MASKED = false>
__global__ void wgrad_reduce_wide_kernel(const float* __restrict__ slab, int64_t lds_, int n_splits, float* __restrict__ dW,
                                         int64_t lddw, float* __restrict__ db, int N, int K, float scale, ReduceArgs<MASKED> m) {
    if constexpr (MODELS) {
        if constexpr (MASKED) {
            if (model_stopped(m)) return;
        }
        slab += nic::linear_model_offset(blockIdx.y, m.slab);
        dW += nic::linear_model_offset(blockIdx.y, m.dW);
        if (db) db += nic::linear_model_offset(blockIdx.y, m.db);
    }
    const int64_t idx = (int64_t)blockIdx.x * (blockDim.x / 64) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (idx >= (int64_t)N * (K + 1)) return;
    const int n = (int)(idx / (K + 1)), k = (int)(idx % (K + 1));
    float s = 0.f;
    for (int sp = lane; sp < n_splits; sp += 64) s += slab[((int64_t)sp * N + n) * lds_ + k];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off);
    if (lane == 0) {
        s *= scale;
        if (k < K) dW[(int64_t)n * lddw + k] = s;
        else if (db) db[n] = s;
    }
}

// ---- forward / input gradient: launches.  WHICH kernel runs, over which grid, is decided in wx_plan.h ---------------------------
// The tuning switches below (and the A/B variants of the dispatch: 1 = 128 x 128 tiles for the big layers, 2 = register-staged
// wgrad, 3 = wgrad without the XCD tile order) exist only in the tuning build tools/gemm_probe.py makes for itself
// (-DNIC_TUNING_BUILD, a separate .so outside the package); the product library has no environment switches: every variant is a
// correct kernel, but which one runs must not depend on a stray variable.
#ifdef NIC_TUNING_BUILD
extern "C" int nic_tuning_set_stamps(void* buf) {  // buf: device memory, 8 x u64 per workgroup of the next launches (or null)
    unsigned long long* pbuf = static_cast<unsigned long long*>(buf);
    return (int)hipMemcpyToSymbol(HIP_SYMBOL(g_nic_stamps), &pbuf, sizeof(pbuf));
}
int env_int(const char* name, int unset) {  // read at every launch
    const char* e = getenv(name);
    return e ? atoi(e) : unset;
}
int wx_lds_pad() { return env_int("NIC_WX_LDS_PAD", 0); }  // unused dynamic LDS per workgroup = fewer co-resident workgroups per CU
int tune_flags() { return env_int("NIC_GEMM_TUNE", 0); }   // timing experiments inside the wx kernel (see WxParams::tune)
int forced_wx_tile() { return env_int("NIC_WX_TILE", -1); }      // tiling id for every wx launch (tools/gemm_tile_probe.py)
int forced_wx_stream() { return env_int("NIC_WX_STREAM", -1); }  // 0 = never, 10 * NT + KS = that instantiation; unset = the picker
int gemm_variant() {
    static int v = env_int("NIC_GEMM_VARIANT", 0);
    return v;
}
nic::WxForce wx_force(const WxParams& p) {   // NIC_WX_TILE in range wins over tune bit 128 (the 256 x 256 tiling)
    const int tile = forced_wx_tile();
    return {forced_wx_stream(), tile >= 0 && tile < 4 ? tile : (p.tune & 128 ? 3 : -1)};
}
constexpr int kWxKernels = nic::WX_KERNEL_END;
#else
constexpr int kWxKernels = nic::WX_PRODUCT_END;   // no force, so no tuning-only kernel: tests/test_wx_plan_host.py
constexpr int wx_lds_pad() { return 0; }
constexpr int tune_flags() { return 0; }
constexpr int gemm_variant() { return 0; }
constexpr nic::WxForce wx_force(const WxParams&) { return {}; }
#endif

// one launcher per kernel family; each holds its template arguments to the kernel's line in nic::kWxGeometry (name, grid, block)
constexpr bool wx_geometry_is(nic::WxKernel id, nic::WxFamily family, int a0, int a1, int a2, int a3, int bm, int bn, int threads) {
    const nic::WxGeometry& g = nic::kWxGeometry[id];
    return g.family == family && g.targs[0] == a0 && g.targs[1] == a1 && g.targs[2] == a2 && g.targs[3] == a3 && g.bm == bm &&
           g.bn == bn && g.threads == threads;
}
template <nic::WxKernel ID, int WM, int WN, int MT, int NT, int EPI>
void launch_wx_dma(const WxParams& p, int grid, hipStream_t s) {
    static_assert(wx_geometry_is(ID, nic::WX_DMA, WM, WN, MT, NT, WM * MT * 32, WN * NT * 32, 64 * WM * WN), "nic::kWxGeometry");
    hipLaunchKernelGGL((gemm_wx_dma_kernel<WM, WN, MT, NT, EPI>), dim3(grid), dim3(64 * WM * WN), wx_lds_pad(), s, p);
}
template <nic::WxKernel ID, int WM, int WN, int MT, int NT, int EPI>
void launch_wx(const WxParams& p, int grid, hipStream_t s) {
    static_assert(wx_geometry_is(ID, nic::WX_STAGED, WM, WN, MT, NT, WM * MT * 32, WN * NT * 32, kThreads), "nic::kWxGeometry");
    hipLaunchKernelGGL((gemm_wx_kernel<WM, WN, MT, NT, EPI>), dim3(grid), dim3(kThreads), 0, s, p);
}
template <nic::WxKernel ID, int NT, int KS, int EPI>
void launch_wx_stream(const WxParams& p, int grid, hipStream_t s) {
    static_assert(wx_geometry_is(ID, nic::WX_STREAM, NT, KS, 0, 0, 32, 32 * NT, 64 * KS), "nic::kWxGeometry");
    hipLaunchKernelGGL((gemm_wx_stream_kernel<NT, KS, EPI>), dim3(grid), dim3(64 * KS), 0, s, p);
}

// the instantiation behind every nic::WxKernel, in the enum's order
template <int EPI>
void (*const kWxLaunch[])(const WxParams&, int grid, hipStream_t) = {
    launch_wx_stream<nic::WX_STREAM_1x2, 1, 2, EPI>, launch_wx_stream<nic::WX_STREAM_1x4, 1, 4, EPI>,
    launch_wx_dma<nic::WX_DMA_128x128, 2, 4, 2, 1, EPI>, launch_wx_dma<nic::WX_DMA_64x128, 2, 4, 1, 1, EPI>,
    launch_wx_dma<nic::WX_DMA_32x128, 1, 4, 1, 1, EPI>,
    launch_wx<nic::WX_STAGED_128x128, 2, 2, 2, 2, EPI>, launch_wx<nic::WX_STAGED_64x128, 1, 4, 2, 1, EPI>,
    launch_wx<nic::WX_STAGED_32x256, 1, 4, 1, 2, EPI>,
#ifdef NIC_TUNING_BUILD
    launch_wx_stream<nic::WX_STREAM_1x1, 1, 1, EPI>, launch_wx_stream<nic::WX_STREAM_2x1, 2, 1, EPI>,
    launch_wx_stream<nic::WX_STREAM_2x2, 2, 2, EPI>, launch_wx_stream<nic::WX_STREAM_2x4, 2, 4, EPI>,
    launch_wx_dma<nic::WX_DMA_256x256, 2, 4, 4, 2, EPI>,
#endif
};

// what nic_last_kernel() reports for each of them: formatted once, by the header
template <int EPI>
struct WxKernelNames {
    char name[kWxKernels][64];
    WxKernelNames() { for (int k = 0; k < kWxKernels; ++k) nic::wx_kernel_name(name[k], sizeof(name[k]), static_cast<nic::WxKernel>(k), epi_name(EPI)); }
};
template <int EPI>
const WxKernelNames<EPI>& wx_kernel_names() {
    static const WxKernelNames<EPI> names;
    return names;
}

template <int EPI>
void dispatch_wx(const WxParams& p, hipStream_t s) {
    const bool operands = nic::wx_operands(reinterpret_cast<uintptr_t>(p.A) | reinterpret_cast<uintptr_t>(p.Bm), p.lda, p.ldb, p.M, p.K);
    const nic::WxPlan plan = nic::wx_plan(p.M, p.K, p.ncols, operands, nic::cu_count(), wx_force(p));
    nic::note_kernel(wx_kernel_names<EPI>().name[plan.kernel]);
    // (asserted here and not next to the array: the array's first use decides where the compiler emits the wx kernels, and they stay
    // behind the weight-gradient kernels, as before the table)
    static_assert(sizeof(kWxLaunch<EPI>) / sizeof(kWxLaunch<EPI>[0]) == kWxKernels, "one launcher per nic::WxKernel this build can plan");
    kWxLaunch<EPI>[plan.kernel](p, plan.grid, s);
}

// ---- weight gradient: launches.  WHICH kernel runs, over which slots, is decided in wgrad_plan.h ----------------------------------
template <int WM, int WN, int MT, int NT>
void launch_wg(const WgParams& p, int n_splits, bool fast, hipStream_t s) {
    constexpr int BM = WM * MT * 32, BN = WN * NT * 32;
    dim3 grid(((p.K + 1 + BN - 1) / BN) * ((p.N + BM - 1) / BM) * n_splits);
    nic::note_kernelf("gemm_wgrad_kernel<%d,%d,%d,%d,%d>", WM, WN, MT, NT, fast ? 1 : 0);
    if (fast) hipLaunchKernelGGL((gemm_wgrad_kernel<WM, WN, MT, NT, 1>), grid, dim3(kThreads), 0, s, p);
    else hipLaunchKernelGGL((gemm_wgrad_kernel<WM, WN, MT, NT, 0>), grid, dim3(kThreads), 0, s, p);
}

template <int WM, int WN, int MT, int NT, bool SKIP = false>
void launch_wg_dma(const WgParams& p, int n_splits, bool, hipStream_t s) {
    constexpr int BM = WM * MT * 32, BN = WN * NT * 32;
    dim3 grid(((p.K + BN - 1) / BN) * ((p.N + BM - 1) / BM) * n_splits);
    nic::note_kernelf(SKIP ? "gemm_wgrad_dma_kernel<%d,%d,%d,%d,skip>" : "gemm_wgrad_dma_kernel<%d,%d,%d,%d>", WM, WN, MT, NT);
    hipLaunchKernelGGL((gemm_wgrad_dma_kernel<WM, WN, MT, NT, SKIP>), grid, dim3(64 * WM * WN), 0, s, p);
}

template <int KC>
void launch_wg_small(const WgParams& p, int n_splits, bool, hipStream_t s) {
    nic::note_kernelf("wgrad_small_kernel<%d>", KC);
    hipLaunchKernelGGL(wgrad_small_kernel<KC>, dim3((n_splits + 3) / 4), dim3(kThreads), 0, s, p, n_splits);
}

// the instantiation behind every nic::WgradTile, in the enum's order
void (*const kWgLaunch[])(const WgParams&, int n_splits, bool fast, hipStream_t) = {
    launch_wg_small<1>, launch_wg_small<2>, launch_wg_small<3>, launch_wg_small<4>,
    launch_wg_dma<8, 1, 2, 2>, launch_wg_dma<4, 2, 2, 2>, launch_wg_dma<2, 4, 2, 2>,                              // tall, half, mid
    launch_wg_dma<4, 2, 1, 5>, launch_wg_dma<4, 2, 1, 6>, launch_wg_dma<4, 2, 1, 7>, launch_wg_dma<2, 4, 2, 2>,   // wide 5-7, big
    launch_wg<2, 2, 2, 2>, launch_wg<2, 2, 2, 1>, launch_wg<1, 4, 2, 1>, launch_wg<1, 4, 1, 2>};
static_assert(sizeof(kWgLaunch) / sizeof(kWgLaunch[0]) == nic::WG_STAGED_32x256 + 1, "one launcher per nic::WgradTile");

int require_ld(const char* who, int32_t n_scenarios, int32_t ldb) {
    NIC_REQUIRE(n_scenarios > 0 && ldb >= n_scenarios && ldb % 4 == 0, "%s: ldb (%d) must be a multiple of 4 and >= n_scenarios (%d)",
                who, ldb, n_scenarios);
    return 0;
}

}  // namespace

extern "C" {

int nic_linear_fwd(const float* W, int64_t ldw, const float* bias, const float* X, float* Y, int32_t N, int32_t K,
                   int32_t n_scenarios, int32_t ldb, int32_t act, void* stream) {
    NIC_REQUIRE(W && X && Y, "nic_linear_fwd: null buffer");
    NIC_REQUIRE(N > 0 && K > 0 && ldw >= K, "nic_linear_fwd: bad N/K/ldw (%d/%d/%lld)", N, K, (long long)ldw);
    NIC_REQUIRE(act == NIC_ACT_NONE || act == NIC_ACT_ELU, "nic_linear_fwd: unknown activation %d", act);
    if (int e = require_ld("nic_linear_fwd", n_scenarios, ldb)) return e;
    NIC_REQUIRE((reinterpret_cast<uintptr_t>(X) & 15) == 0 && (reinterpret_cast<uintptr_t>(Y) & 15) == 0,
                "nic_linear_fwd: X/Y must be 16-byte aligned");
    WxParams p{W, ldw, X, Y, bias, nullptr, N, K, (n_scenarios + 3) / 4 * 4, ldb, act, 0, tune_flags()};
    dispatch_wx<EPI_BIAS_ACT>(p, nic::as_stream(stream));
    return nic::check_launch("nic_linear_fwd");
}

int nic_linear_dgrad(const float* Wt, int64_t ldwt, const float* dY, const float* Hprev, float* dX, int32_t N, int32_t K,
                     int32_t n_scenarios, int32_t ldb, int32_t act_prev, int32_t accumulate, void* stream) {
    NIC_REQUIRE(Wt && dY && dX, "nic_linear_dgrad: null buffer");
    NIC_REQUIRE(N > 0 && K > 0 && ldwt >= N, "nic_linear_dgrad: bad N/K/ldwt (%d/%d/%lld)", N, K, (long long)ldwt);
    if (int e = require_ld("nic_linear_dgrad", n_scenarios, ldb)) return e;
    NIC_REQUIRE((reinterpret_cast<uintptr_t>(dY) & 15) == 0 && (reinterpret_cast<uintptr_t>(dX) & 15) == 0,
                "nic_linear_dgrad: dY/dX must be 16-byte aligned");
    // dX[K][b] = Wt[K][N] * dY[N][b]: output rows = K, contraction = N
    WxParams p{Wt, ldwt, dY, dX, nullptr, Hprev, K, N, (n_scenarios + 3) / 4 * 4, ldb, act_prev, accumulate, tune_flags()};
    dispatch_wx<EPI_DGRAD>(p, nic::as_stream(stream));
    return nic::check_launch("nic_linear_dgrad");
}

int nic_wgrad_num_splits(int32_t N, int32_t K, int32_t n_scenarios) {
    return nic::wgrad_recommended_slots(N, K, n_scenarios, nic::cu_count());
}
int nic_wgrad_periods_num_splits(int32_t N, int32_t K, int32_t n_scenarios, int32_t n_periods) {
    return nic::wgrad_periods_recommended_slots(N, K, n_scenarios, n_periods, nic::cu_count());
}

// nic_linear_wgrad (one period) and nic_linear_wgrad_periods: argument checks, the plan (wgrad_plan.h), its launches
static int wgrad_run(nic::WgradEntry entry, const float* dY, const float* X, float* slab, int64_t lds_, int32_t N, int32_t K,
                     int32_t n_scenarios, int32_t ldb, int32_t n_splits, int32_t n_periods, int64_t pstride_dy, int64_t pstride_x,
                     void* stream, const char* who) {
    NIC_REQUIRE(dY && X && slab, "%s: null buffer", who);
    NIC_REQUIRE(N > 0 && K > 0 && lds_ >= K + 1, "%s: bad N/K/lds (%d/%d/%lld)", who, N, K, (long long)lds_);
    NIC_REQUIRE(n_splits >= 1, "%s: n_splits must be >= 1", who);
    if (int e = require_ld(who, n_scenarios, ldb)) return e;
    const nic::WgradOperands operands = nic::wgrad_operands(reinterpret_cast<uintptr_t>(dY) | reinterpret_cast<uintptr_t>(X),
                                                            reinterpret_cast<uintptr_t>(slab), ldb, lds_, N, K);
    const nic::WgradPlan plan = nic::wgrad_plan(entry, N, K, n_scenarios, n_periods, n_splits, operands, gemm_variant() == 2);
    const bool calls = plan.cut == nic::WG_PER_PERIOD;   // nic_linear_wgrad calls: no period strides, launch errors under that name
    if (!calls && entry == nic::WG_ALL_PERIODS) who = "nic_linear_wgrad_periods";
    for (nic::WgradLaunch l = nic::wgrad_launch(plan, n_periods, 0); l.n_periods > 0;
         l = nic::wgrad_launch(plan, n_periods, l.first_period + l.n_periods)) {
        WgParams p{dY + l.first_period * pstride_dy, X + l.first_period * pstride_x, slab, lds_, ldb, N, K, n_scenarios, plan.chunk,
                   gemm_variant() == 3 ? 0 : 1, l.n_periods, calls ? 0 : pstride_dy, calls ? 0 : pstride_x, plan.flush_periods,
                   plan.scen_splits, plan.periods_per_group};
        kWgLaunch[l.tile](p, plan.slots, operands.buffer, nic::as_stream(stream));
        if (int e = nic::check_launch(who)) return e;
    }
    return 0;
}

int nic_linear_wgrad(const float* dY, const float* X, float* slab, int64_t lds_, int32_t N, int32_t K, int32_t n_scenarios,
                     int32_t ldb, int32_t n_splits, void* stream) {
    return wgrad_run(nic::WG_ONE_PERIOD, dY, X, slab, lds_, N, K, n_scenarios, ldb, n_splits, 1, 0, 0, stream, "nic_linear_wgrad");
}

int nic_linear_wgrad_periods(const float* dY, const float* X, float* slab, int64_t lds_, int32_t N, int32_t K,
                             int32_t n_scenarios, int32_t ldb, int32_t n_splits, int32_t n_periods, int64_t period_stride_dy,
                             int64_t period_stride_x, void* stream) {
    NIC_REQUIRE(n_periods >= 1, "nic_linear_wgrad_periods: n_periods must be >= 1");
    // Periods are accumulated LAST FIRST, the order autograd accumulates them in the reference: pre-activation gradients grow
    // towards the start of the horizon (each period adds the costs it influences later), so this sums the small terms
    // before the large ones.  Measured at 512x3, T = 100: bias-gradient error against an fp64 evaluation 2.9e-5 in
    // ascending order, 1e-6 descending.
    if (n_periods > 1) {
        dY += (int64_t)(n_periods - 1) * period_stride_dy;
        X += (int64_t)(n_periods - 1) * period_stride_x;
        period_stride_dy = -period_stride_dy;
        period_stride_x = -period_stride_x;
    }
    NIC_REQUIRE(period_stride_dy % 4 == 0 && period_stride_x % 4 == 0,
                "nic_linear_wgrad_periods: period strides must be multiples of 4 elements (16-byte aligned operands)");
    // (a horizon of one period and the tiny layers ran as nic_linear_wgrad calls: argument errors come under that name)
    const char* who = n_periods == 1 || (N <= 32 && K <= 32) ? "nic_linear_wgrad" : "nic_linear_wgrad_periods";
    return wgrad_run(nic::WG_ALL_PERIODS, dY, X, slab, lds_, N, K, n_scenarios, ldb, n_splits, n_periods, period_stride_dy,
                     period_stride_x, stream, who);
}

int nic_wgrad_reduce(const float* slab, int64_t lds_, int32_t n_splits, float* dW, int64_t lddw, float* db, int32_t N,
                     int32_t K, float scale, void* stream) {
    NIC_REQUIRE(slab && dW, "nic_wgrad_reduce: null buffer");
    NIC_REQUIRE(N > 0 && K > 0 && lds_ >= K + 1 && lddw >= K && n_splits >= 1, "nic_wgrad_reduce: bad sizes");
    const int64_t total = (int64_t)N * (K + 1);
    const bool wide = nic::wgrad_reduce_wide(n_splits, N, K);
    nic::note_kernel(wide ? "wgrad_reduce_wide_kernel" : "wgrad_reduce_kernel");
    if (wide)
        hipLaunchKernelGGL(wgrad_reduce_wide_kernel<false>, dim3(nic::ceil_div(total, 4)), dim3(256), 0, nic::as_stream(stream), slab,
                           lds_, n_splits, dW, lddw, db, N, K, scale, ReduceModels{});
    else
        hipLaunchKernelGGL(wgrad_reduce_kernel<false>, dim3(nic::ceil_div(total, 256)), dim3(256), 0, nic::as_stream(stream), slab, lds_,
                           n_splits, dW, lddw, db, N, K, scale, ReduceModels{});
    return nic::check_launch("nic_wgrad_reduce");
}

}  // extern "C"

namespace {

// ---- model forms: the MODELS instantiation of the same kernel over dim3(the single-model grid, n_models) --------------------------
// (defined HERE, behind the single-model entry points: the tables below are the first use of the model kernels, so they are emitted
// behind the single-model ones, whose order in the code object stays what it was)
// MASKED: the twin that tests p.active (the _active entry points); else the kernel as it was, on the parameters without the mask
template <bool MASKED> const WxArgs<MASKED>& wx_args(const WxModelParams& p) { return p; }
template <bool MASKED> const WgArgs<MASKED>& wg_args(const WgModelParams& p) { return p; }
template <bool MASKED, int WM, int WN, int MT, int NT, int EPI = EPI_BIAS_ACT>
void launch_wx_dma_models(const WxModelParams& p, int grid, int n_models, hipStream_t s) {
    hipLaunchKernelGGL((gemm_wx_dma_kernel<WM, WN, MT, NT, EPI, true, MASKED>), dim3(grid, n_models), dim3(64 * WM * WN), wx_lds_pad(), s,
                       wx_args<MASKED>(p));
}
template <bool MASKED, int WM, int WN, int MT, int NT, int EPI = EPI_BIAS_ACT>
void launch_wx_models(const WxModelParams& p, int grid, int n_models, hipStream_t s) {
    hipLaunchKernelGGL((gemm_wx_kernel<WM, WN, MT, NT, EPI, true, MASKED>), dim3(grid, n_models), dim3(kThreads), 0, s, wx_args<MASKED>(p));
}
template <bool MASKED, int NT, int KS, int EPI = EPI_BIAS_ACT>
void launch_wx_stream_models(const WxModelParams& p, int grid, int n_models, hipStream_t s) {
    hipLaunchKernelGGL((gemm_wx_stream_kernel<NT, KS, EPI, true, MASKED>), dim3(grid, n_models), dim3(64 * KS), 0, s, wx_args<MASKED>(p));
}
// in nic::WxKernel's order, with kWxLaunch's template arguments; null: no model form (nic::lm_wx_has_model_form refuses the request)
// (forwards only: nothing asks for a model form of the input gradient)
template <bool MASKED>
void (*const kWxLaunchModels[nic::WX_PRODUCT_END])(const WxModelParams&, int grid, int n_models, hipStream_t) = {
    launch_wx_stream_models<MASKED, 1, 2>, launch_wx_stream_models<MASKED, 1, 4>,
    nullptr, launch_wx_dma_models<MASKED, 2, 4, 1, 1>, launch_wx_dma_models<MASKED, 1, 4, 1, 1>,
    nullptr, launch_wx_models<MASKED, 1, 4, 2, 1>, launch_wx_models<MASKED, 1, 4, 1, 2>,
};

template <bool MASKED, int WM, int WN, int MT, int NT>
void launch_wg_models(const WgModelParams& p, int n_splits, bool fast, int n_models, hipStream_t s) {
    constexpr int BM = WM * MT * 32, BN = WN * NT * 32;
    dim3 grid(((p.K + 1 + BN - 1) / BN) * ((p.N + BM - 1) / BM) * n_splits, n_models);
    nic::note_kernelf("gemm_wgrad_kernel<%d,%d,%d,%d,%d,models=%d%s>", WM, WN, MT, NT, fast ? 1 : 0, n_models, MASKED ? ",active" : "");
    if (fast) hipLaunchKernelGGL((gemm_wgrad_kernel<WM, WN, MT, NT, 1, true, MASKED>), grid, dim3(kThreads), 0, s, wg_args<MASKED>(p));
    else hipLaunchKernelGGL((gemm_wgrad_kernel<WM, WN, MT, NT, 0, true, MASKED>), grid, dim3(kThreads), 0, s, wg_args<MASKED>(p));
}
template <bool MASKED, int KC>
void launch_wg_small_models(const WgModelParams& p, int n_splits, bool, int n_models, hipStream_t s) {
    nic::note_kernelf("wgrad_small_kernel<%d,models=%d%s>", KC, n_models, MASKED ? ",active" : "");
    hipLaunchKernelGGL((wgrad_small_kernel<KC, true, MASKED>), dim3((n_splits + 3) / 4, n_models), dim3(kThreads), 0, s, wg_args<MASKED>(p),
                       n_splits);
}
// in nic::WgradTile's order, with kWgLaunch's template arguments; null: the LDS-DMA tiles (nic::lm_wgrad_has_model_form)
template <bool MASKED>
void (*const kWgLaunchModels[nic::WG_STAGED_32x256 + 1])(const WgModelParams&, int n_splits, bool fast, int n_models, hipStream_t) = {
    launch_wg_small_models<MASKED, 1>, launch_wg_small_models<MASKED, 2>, launch_wg_small_models<MASKED, 3>, launch_wg_small_models<MASKED, 4>,
    nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
    launch_wg_models<MASKED, 2, 2, 2, 2>, launch_wg_models<MASKED, 2, 2, 2, 1>, launch_wg_models<MASKED, 1, 4, 2, 1>,
    launch_wg_models<MASKED, 1, 4, 1, 2>};

}  // namespace

extern "C" {

// ---- K models in one launch (csrc/linear_models_plan.h: checks and plan; grid y = model) ----------------------------------------
// nic_last_kernel: the single-model kernel's name with ",models=K>" in place of the closing ">"; the two reduce kernels have no
// template list and get the suffix ",models=K" appended.
// (`masked`: through an _active entry point - `active` is checked, the MASKED twins run and nic_last_kernel says so)
static int fwd_models_run(const char* who, bool masked, const float* W, int64_t ldw, int64_t W_stride, const float* bias, int64_t bias_stride,
                          const float* X, int64_t X_stride, float* Y, int64_t Y_stride, int32_t N, int32_t K, int32_t n_scenarios,
                          int32_t ldb, int32_t act, int32_t n_models, const int32_t* active, void* stream) {
    const nic::LmFwdRequest r{reinterpret_cast<uintptr_t>(W), reinterpret_cast<uintptr_t>(bias), reinterpret_cast<uintptr_t>(X),
                              reinterpret_cast<uintptr_t>(Y), ldw, W_stride, bias_stride, X_stride, Y_stride, N, K, n_scenarios, ldb,
                              act, n_models, reinterpret_cast<uintptr_t>(active)};
    const WxModelParams p{{W, ldw, X, Y, bias, nullptr, N, K, (n_scenarios + 3) / 4 * 4, ldb, act, 0, tune_flags(), W_stride, X_stride,
                           Y_stride, bias_stride}, active};
    const nic::LmFwdPlan plan = nic::linear_models_fwd_plan(r, nic::cu_count(), wx_force(p));
    NIC_REQUIRE(plan.refusal == nic::LM_OK, "%s: %s", who, nic::linear_models_reason(plan.refusal));
    const char* name = wx_kernel_names<EPI_BIAS_ACT>().name[plan.plan.kernel];
    nic::note_kernelf("%.*s,models=%d%s>", (int)strlen(name) - 1, name, n_models, masked ? ",active" : "");
    (masked ? kWxLaunchModels<true> : kWxLaunchModels<false>)[plan.plan.kernel](p, plan.plan.grid, n_models, nic::as_stream(stream));
    return nic::check_launch(who);
}
int nic_linear_fwd_models(const float* W, int64_t ldw, int64_t W_stride, const float* bias, int64_t bias_stride, const float* X,
                          int64_t X_stride, float* Y, int64_t Y_stride, int32_t N, int32_t K, int32_t n_scenarios, int32_t ldb,
                          int32_t act, int32_t n_models, void* stream) {
    return fwd_models_run("nic_linear_fwd_models", false, W, ldw, W_stride, bias, bias_stride, X, X_stride, Y, Y_stride, N, K, n_scenarios,
                          ldb, act, n_models, nullptr, stream);
}

static int wgrad_models_run(const char* who, bool masked, const float* dY, int64_t dY_stride, const float* X, int64_t X_stride, float* slab,
                            int64_t slab_stride, int64_t lds_, int32_t N, int32_t K, int32_t n_scenarios, int32_t ldb, int32_t n_splits,
                            int32_t n_models, const int32_t* active, void* stream) {
    const nic::LmWgradRequest r{reinterpret_cast<uintptr_t>(dY), reinterpret_cast<uintptr_t>(X), reinterpret_cast<uintptr_t>(slab),
                                dY_stride, X_stride, slab_stride, lds_, N, K, n_scenarios, ldb, n_splits, n_models,
                                reinterpret_cast<uintptr_t>(active)};
    const nic::LmWgradPlan lm = nic::linear_models_wgrad_plan(r, gemm_variant() == 2);
    NIC_REQUIRE(lm.refusal == nic::LM_OK, "%s: %s", who, nic::linear_models_reason(lm.refusal));
    const nic::WgradPlan& plan = lm.plan;
    const nic::WgradLaunch l = nic::wgrad_launch(plan, 1, 0);   // (nic_linear_wgrad's one launch)
    const WgModelParams p{{dY, X, slab, lds_, ldb, N, K, n_scenarios, plan.chunk, gemm_variant() == 3 ? 0 : 1, l.n_periods, 0, 0,
                           plan.flush_periods, plan.scen_splits, plan.periods_per_group, dY_stride, X_stride, slab_stride}, active};
    (masked ? kWgLaunchModels<true> : kWgLaunchModels<false>)[l.tile](p, plan.slots, lm.operands.buffer, n_models, nic::as_stream(stream));
    return nic::check_launch(who);
}
int nic_linear_wgrad_models(const float* dY, int64_t dY_stride, const float* X, int64_t X_stride, float* slab, int64_t slab_stride,
                            int64_t lds_, int32_t N, int32_t K, int32_t n_scenarios, int32_t ldb, int32_t n_splits, int32_t n_models,
                            void* stream) {
    return wgrad_models_run("nic_linear_wgrad_models", false, dY, dY_stride, X, X_stride, slab, slab_stride, lds_, N, K, n_scenarios, ldb,
                            n_splits, n_models, nullptr, stream);
}

static int reduce_models_run(const char* who, bool masked, const float* slab, int64_t slab_stride, int64_t lds_, int32_t n_splits, float* dW,
                             int64_t lddw, int64_t dW_stride, float* db, int64_t db_stride, int32_t N, int32_t K, float scale,
                             int32_t n_models, const int32_t* active, void* stream) {
    const nic::LmReduceRequest r{reinterpret_cast<uintptr_t>(slab), reinterpret_cast<uintptr_t>(dW), reinterpret_cast<uintptr_t>(db),
                                 slab_stride, lds_, lddw, dW_stride, db_stride, N, K, n_splits, n_models,
                                 reinterpret_cast<uintptr_t>(active)};
    const int refusal = nic::linear_models_check_reduce(r);
    NIC_REQUIRE(refusal == nic::LM_OK, "%s: %s", who, nic::linear_models_reason(refusal));
    const int64_t total = (int64_t)N * (K + 1);
    const bool wide = nic::wgrad_reduce_wide(n_splits, N, K);
    nic::note_kernelf("%s,models=%d%s", wide ? "wgrad_reduce_wide_kernel" : "wgrad_reduce_kernel", n_models, masked ? ",active" : "");
    const ReduceModelStrides m{{slab_stride, dW_stride, db_stride}, active};
    const ReduceModels& unmasked = m;
    const dim3 grid(wide ? nic::ceil_div(total, 4) : nic::ceil_div(total, 256), n_models);
    hipStream_t s = nic::as_stream(stream);
    if (wide && masked)
        hipLaunchKernelGGL((wgrad_reduce_wide_kernel<true, true>), grid, dim3(256), 0, s, slab, lds_, n_splits, dW, lddw, db, N, K, scale, m);
    else if (wide)
        hipLaunchKernelGGL((wgrad_reduce_wide_kernel<true>), grid, dim3(256), 0, s, slab, lds_, n_splits, dW, lddw, db, N, K, scale, unmasked);
    else if (masked)
        hipLaunchKernelGGL((wgrad_reduce_kernel<true, true>), grid, dim3(256), 0, s, slab, lds_, n_splits, dW, lddw, db, N, K, scale, m);
    else
        hipLaunchKernelGGL((wgrad_reduce_kernel<true>), grid, dim3(256), 0, s, slab, lds_, n_splits, dW, lddw, db, N, K, scale, unmasked);
    return nic::check_launch(who);
}
int nic_wgrad_reduce_models(const float* slab, int64_t slab_stride, int64_t lds_, int32_t n_splits, float* dW, int64_t lddw,
                            int64_t dW_stride, float* db, int64_t db_stride, int32_t N, int32_t K, float scale, int32_t n_models,
                            void* stream) {
    return reduce_models_run("nic_wgrad_reduce_models", false, slab, slab_stride, lds_, n_splits, dW, lddw, dW_stride, db, db_stride, N, K,
                             scale, n_models, nullptr, stream);
}

/* ---- the same three under the active-model mask (csrc/linear_models_plan.h): a model whose entry is zero is not run: none of its
   operands is read, none of its outputs written.  The plan, the kernels and an active model's bits are the unmasked call's.
   nic_last_kernel: the unmasked name with ",active" behind "models=K". ---- */
int nic_linear_fwd_models_active(const float* W, int64_t ldw, int64_t W_stride, const float* bias, int64_t bias_stride, const float* X,
                                 int64_t X_stride, float* Y, int64_t Y_stride, int32_t N, int32_t K, int32_t n_scenarios, int32_t ldb,
                                 int32_t act, int32_t n_models, const int32_t* active, void* stream) {
    return fwd_models_run("nic_linear_fwd_models_active", true, W, ldw, W_stride, bias, bias_stride, X, X_stride, Y, Y_stride, N, K,
                          n_scenarios, ldb, act, n_models, active, stream);
}
int nic_linear_wgrad_models_active(const float* dY, int64_t dY_stride, const float* X, int64_t X_stride, float* slab, int64_t slab_stride,
                                   int64_t lds_, int32_t N, int32_t K, int32_t n_scenarios, int32_t ldb, int32_t n_splits,
                                   int32_t n_models, const int32_t* active, void* stream) {
    return wgrad_models_run("nic_linear_wgrad_models_active", true, dY, dY_stride, X, X_stride, slab, slab_stride, lds_, N, K, n_scenarios,
                            ldb, n_splits, n_models, active, stream);
}
int nic_wgrad_reduce_models_active(const float* slab, int64_t slab_stride, int64_t lds_, int32_t n_splits, float* dW, int64_t lddw,
                                   int64_t dW_stride, float* db, int64_t db_stride, int32_t N, int32_t K, float scale, int32_t n_models,
                                   const int32_t* active, void* stream) {
    return reduce_models_run("nic_wgrad_reduce_models_active", true, slab, slab_stride, lds_, n_splits, dW, lddw, dW_stride, db, db_stride,
                             N, K, scale, n_models, active, stream);
}

// 1 if the model forms take a layer as the engines allocate it (16-byte aligned operands, leading dimensions multiples of 4):
// wgrad = 0: the forward of N x K over n_scenarios columns; wgrad = 1: the one-period weight gradient of N x K with
// nic_wgrad_num_splits(N, K, n_scenarios) splits.  Launches nothing; no device access besides the compute-unit count.
int nic_linear_models_ok(int32_t N, int32_t K, int32_t n_scenarios, int32_t ldb, int32_t n_models, int32_t wgrad) {
    const int64_t lda = (K + 3) / 4 * 4;
    if (wgrad) {
        const int n_splits = nic::wgrad_recommended_slots(N, K, n_scenarios, nic::cu_count());
        const int64_t lds_ = (K + 1 + 3) / 4 * 4;
        const nic::LmWgradRequest r{16, 16, 16, (int64_t)N * ldb, (int64_t)K * ldb, (int64_t)(n_splits > 0 ? n_splits : 1) * N * lds_, lds_,
                                    N, K, n_scenarios, ldb, n_splits, n_models};
        return nic::linear_models_wgrad_plan(r).refusal == nic::LM_OK;
    }
    const nic::LmFwdRequest r{16, 16, 16, 16, lda, (int64_t)N * lda, N, 0, (int64_t)N * ldb, N, K, n_scenarios, ldb, NIC_ACT_NONE, n_models};
    return nic::linear_models_fwd_plan(r, nic::cu_count()).refusal == nic::LM_OK;
}
}
