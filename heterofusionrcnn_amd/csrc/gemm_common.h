// gemm_common.h -- the tile machine shared by the MFMA GEMM sources (gemm.hip, fp_linear.hip): the guarded staging load, the
// pieces of the forward form (LDS layout, staging geometry, the MFMA stage fwd_mfma_stage, the D-register row map, the column-sum
// epilogue col_sums_store), the wgrad-form chunk loop (wgrad_tile_loop), and the launch plans that both the launchers and the
// workspace queries must agree on.  fwd_mfma_stage and wgrad_tile_loop hold the only MFMA calls of those sources.  The three wgrad
// kernels are an operand source handed to wgrad_tile_loop (conv_nhwc.hip's, which masks its G operand, to wgrad_tile_loop_staged).  The five forward kernels keep their own loop over tiles and stages
// around fwd_mfma_stage: through one shared forward loop (fetch / stage functors) their register allocation moved by up to 45
// VGPRs, scratch grew in four instantiations, and the lifting kernels ran 3-8 % slower on the benchmark's shapes
// (profiles/gemm_refactor_ab.md, last section, which also says why a tile's accumulator zeroing stays written out in each).
#pragma once
#include <stdint.h>

#include "hf_common.h"

namespace hf {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kGemmThreads = 256;
constexpr int kGemmRowsPerStage = 32;  // rows staged in LDS per step = 16 MFMA k-pairs

// four consecutive floats of row `row`, zero outside [0, row_end) x [0, ncols).  Branch-free: an out-of-range
// access reads a safe address and is replaced by zero afterwards.  VEC: ncols % 4 == 0 and a 16-byte aligned base.
template <bool VEC>
__device__ __forceinline__ float4 load4_guarded(const float *__restrict__ base, long long row, long long row_end,
                                                int col, int ncols)
{
    const bool row_ok = row < row_end;
    const float *p = base + (row_ok ? row : 0) * ncols;
    if constexpr (VEC) {
        const bool ok = row_ok && col < ncols;
        const float4 v = *reinterpret_cast<const float4 *>(p + (ok ? col : 0));
        return ok ? v : make_float4(0.f, 0.f, 0.f, 0.f);
    } else {
        float4 v;
        const bool k0 = row_ok && col < ncols, k1 = row_ok && col + 1 < ncols, k2 = row_ok && col + 2 < ncols,
                   k3 = row_ok && col + 3 < ncols;
        const float x = p[k0 ? col : 0], y = p[k1 ? col + 1 : 0], z = p[k2 ? col + 2 : 0], w = p[k3 ? col + 3 : 0];
        v.x = k0 ? x : 0.f; v.y = k1 ? y : 0.f; v.z = k2 ? z : 0.f; v.w = k3 ? w : 0.f;
        return v;
    }
}

// ------------------------------------------------------------------------------------------
// v_mfma_f32_32x32x2_f32 lane maps (lane l): A[i = l&31][k = l>>5], B[k = l>>5][j = l&31];
// D register g holds row i = 8*(g>>2) + 4*(l>>5) + (g&3), column j = l&31 of the 32x32 tile.
// ------------------------------------------------------------------------------------------
// the matrix row of D register g, `tile_row` being the row of the 32x32 tile's first.  The sum is formed in tile_row's type and in
// this order: with 64-bit rows the compiler then derives the sixteen store addresses of a lane from one base
template <class Row>
__device__ __forceinline__ Row mfma_d_row(Row tile_row, int g, int lane) { return tile_row + 8 * (g >> 2) + 4 * (lane >> 5) + (g & 3); }

// ------------------------------------------------------------------------------------------
// Forward form: Z (R, N) = A (R, K) B^T (N, K), a workgroup owns 128 rows and all N <= 256 columns; wave w holds rows
// 32w .. 32w+31 as NT = ceil(N / 32) accumulator tiles.
// ------------------------------------------------------------------------------------------
constexpr int kFwdRows = 128;   // rows per workgroup tile
constexpr int kFwdKC = 32;      // input channels per LDS stage
constexpr int kFwdLS = kFwdKC + 4;  // LDS row stride (keeps float4 stores aligned; 2-way read conflicts are noise here)

template <int NT, int NV = 2>
struct alignas(16) FwdLds {
    float As[kFwdRows * kFwdLS];
    float Bs[NT * 32 * kFwdLS];
    float red[4][NT * 32][NV];  // col_sums_store
};

// staging: 8 threads cover the 32 channels of a row, 32 rows per pass -> thread t stages channels fwd_k4() .. +3 of rows
// fwd_srow() + 32 p, p < 4 (A) and p < NT (B)
__device__ __forceinline__ int fwd_k4() { return (threadIdx.x & 7) * 4; }
__device__ __forceinline__ int fwd_srow() { return threadIdx.x >> 3; }
// row of D register g in the tile that starts at row0: wave w holds rows 32w .. 32w+31
__device__ __forceinline__ long long fwd_d_row(long long row0, int g) { return mfma_d_row(row0 + 32 * (threadIdx.x >> 6), g, threadIdx.x & 63); }

// the MFMAs of one staged 32-channel stage, between the two barriers of a stage.  A kernel stores the stage (thread t: four
// floats per pass into As and Bs, see fwd_k4 / fwd_srow), synchronises, issues the global loads of the NEXT stage -- of this tile,
// or the first one of the workgroup's next tile -- so that they are in flight during the MFMAs and the epilogue's stores, and
// calls this
template <int NT, int NV>
__device__ __forceinline__ void fwd_mfma_stage(const FwdLds<NT, NV> &lds, f32x16 (&acc)[NT])
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float *ap = lds.As + (32 * wave + (lane & 31)) * kFwdLS + (lane >> 5);
    const float *bp = lds.Bs + (lane & 31) * kFwdLS + (lane >> 5);
#pragma unroll 4
    for (int s = 0; s < kFwdKC / 2; ++s) {
        const float a = ap[2 * s];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
            acc[nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bp[nt * 32 * kFwdLS + 2 * s], acc[nt], 0, 0, 0);
    }
}

// per-workgroup column sums of NV values per column (the BatchNorm partial-sum layout of hf_common.h, NV blocks of ncols
// channels): the two row-halves of a wave, then the four waves in a fixed order
template <int NT, int NV>
__device__ __forceinline__ void col_sums_store(FwdLds<NT, NV> &lds, float (&s)[NT][NV], int ncols, float *__restrict__ partial)
{
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            s[nt][v] += __shfl_xor(s[nt][v], 32);
            if (lane < 32) lds.red[wave][nt * 32 + lane][v] = s[nt][v];
        }
    __syncthreads();
    for (int col = t; col < ncols; col += kGemmThreads) {
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            float a = lds.red[0][col][v];
#pragma unroll
            for (int w = 1; w < 4; ++w) a += lds.red[w][col][v];
            partial[(static_cast<size_t>(v) * ncols + col) * kBnMaxBlocks + blockIdx.x] = a;
        }
    }
}

// ------------------------------------------------------------------------------------------
// Wgrad form: partial[chunk][n][k] = sum over the chunk's rows of G[r][n] * X[r][k]; the reduction runs over rows, both operands
// are staged in their row-major layout.  WM / WN: 32x32 MFMA tiles per wave along n / k; a workgroup is 2 x 2 waves and owns the
// 64 WM x 64 WN output tile (blockIdx.x) of one chunk of rows (blockIdx.y).
// ------------------------------------------------------------------------------------------
template <int WM, int WN>
struct WgradTile {
    static constexpr int TM = 64 * WM, TN = 64 * WN;
    static constexpr int GS = TM + 32, XS = TN + 32;  // LDS row strides: the two row-halves of a wave land on disjoint banks
    static constexpr int GC4 = TM / 4, XC4 = TN / 4;  // float4 per staged row
    static constexpr int GPASS = kGemmRowsPerStage * GC4 / kGemmThreads, XPASS = kGemmRowsPerStage * XC4 / kGemmThreads;
    static constexpr int GROWS = kGemmThreads / GC4, XROWS = kGemmThreads / XC4;  // rows covered per pass
    struct alignas(16) Lds {
        float Gs[kGemmRowsPerStage * GS];
        float Xs[kGemmRowsPerStage * XS];
    };
    // this thread's share of a stage: columns gcol .. +3 of G rows rt + grow + p GROWS (p < GPASS), columns xcol .. +3 of X rows
    // rt + xrow + p XROWS (p < XPASS); [r0, r1) are the workgroup's rows
    int tile_m, tile_n, gcol, grow, xcol, xrow;
    long long r0, r1;
    __device__ __forceinline__ WgradTile(long long rows, int mtiles, long long rows_per_chunk)
    {
        const int t = threadIdx.x;
        tile_m = blockIdx.x % mtiles; tile_n = blockIdx.x / mtiles;
        r0 = blockIdx.y * rows_per_chunk;
        r1 = r0 + rows_per_chunk < rows ? r0 + rows_per_chunk : rows;
        gcol = tile_m * TM + (t % GC4) * 4; grow = t / GC4;
        xcol = tile_n * TN + (t % XC4) * 4; xrow = t / XC4;
    }
};

// The chunk loop.  fetch(rt) issues the loads of the stage at row rt; stage_g(p) and stage_x(p, rt) give the four floats to store in
// Gs and Xs for pass p from what fetch loaded -- evaluated when the stage is stored, so the loads stay in flight across the MFMA loop.
template <int WM, int WN, class Fetch, class StageG, class StageX>
__device__ __forceinline__ void wgrad_tile_loop_staged(typename WgradTile<WM, WN>::Lds &lds, const WgradTile<WM, WN> &q, int cout, int cin,
                                                       float *__restrict__ partial, Fetch fetch, StageG stage_g, StageX stage_x)
{
    using T = WgradTile<WM, WN>;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int wm = wave & 1, wn = wave >> 1;
    f32x16 acc[WM][WN];
#pragma unroll
    for (int i = 0; i < WM; ++i)
#pragma unroll
        for (int j = 0; j < WN; ++j)
#pragma unroll
            for (int g = 0; g < 16; ++g) acc[i][j][g] = 0.f;

    fetch(q.r0);
    for (long long rt = q.r0; rt < q.r1; rt += kGemmRowsPerStage) {
#pragma unroll
        for (int p = 0; p < T::GPASS; ++p)
            *reinterpret_cast<float4 *>(&lds.Gs[(q.grow + p * T::GROWS) * T::GS + (t % T::GC4) * 4]) = stage_g(p);
#pragma unroll
        for (int p = 0; p < T::XPASS; ++p)
            *reinterpret_cast<float4 *>(&lds.Xs[(q.xrow + p * T::XROWS) * T::XS + (t % T::XC4) * 4]) = stage_x(p, rt);
        __syncthreads();
        if (rt + kGemmRowsPerStage < q.r1) fetch(rt + kGemmRowsPerStage);  // in flight during the MFMAs below
        const float *ga = lds.Gs + (lane >> 5) * T::GS + wm * 32 * WM + (lane & 31);
        const float *xb = lds.Xs + (lane >> 5) * T::XS + wn * 32 * WN + (lane & 31);
        float a[2][WM], b[2][WN];  // operands of the next row pair are read while this pair's MFMAs run
#pragma unroll
        for (int i = 0; i < WM; ++i) a[0][i] = ga[i * 32];
#pragma unroll
        for (int j = 0; j < WN; ++j) b[0][j] = xb[j * 32];
#pragma unroll
        for (int s = 0; s < kGemmRowsPerStage / 2; ++s) {
            const int cur = s & 1, nxt = cur ^ 1;
            if (s + 1 < kGemmRowsPerStage / 2) {
#pragma unroll
                for (int i = 0; i < WM; ++i) a[nxt][i] = ga[2 * (s + 1) * T::GS + i * 32];
#pragma unroll
                for (int j = 0; j < WN; ++j) b[nxt][j] = xb[2 * (s + 1) * T::XS + j * 32];
            }
#pragma unroll
            for (int i = 0; i < WM; ++i)
#pragma unroll
                for (int j = 0; j < WN; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[cur][i], b[cur][j], acc[i][j], 0, 0, 0);
        }
        __syncthreads();
    }

    float *out = partial + static_cast<size_t>(blockIdx.y) * cout * cin;
#pragma unroll
    for (int i = 0; i < WM; ++i)
#pragma unroll
        for (int j = 0; j < WN; ++j) {
            const int k = q.tile_n * T::TN + wn * 32 * WN + j * 32 + (lane & 31);
#pragma unroll
            for (int g = 0; g < 16; ++g) {
                const int n = mfma_d_row(q.tile_m * T::TM + wm * 32 * WM + i * 32, g, lane);
                if (n < cout && k < cin) out[static_cast<size_t>(n) * cin + k] = acc[i][j][g];
            }
        }
}

// The loop with G stored as loaded: gr[] is the kernel's own array, which fetch overwrites through its captures; the loop only reads
// it, after each fetch.
template <int WM, int WN, class Fetch, class StageX>
__device__ __forceinline__ void wgrad_tile_loop(typename WgradTile<WM, WN>::Lds &lds, const WgradTile<WM, WN> &q, int cout, int cin,
                                                float *__restrict__ partial,
                                                const float4 (&gr)[WgradTile<WM, WN>::GPASS], Fetch fetch, StageX stage_x)
{
    wgrad_tile_loop_staged<WM, WN>(lds, q, cout, cin, partial, fetch, [&](int p) { return gr[p]; }, stage_x);
}

struct WgradPlan {
    int wm, wn, mtiles, ntiles, chunks;
    long long rows_per_chunk;
};

inline WgradPlan wgrad_plan(long long rows, int cout, int cin)
{
    WgradPlan p;
    p.wm = cout > 64 ? 2 : 1;
    p.wn = cin > 64 ? 2 : 1;
    p.mtiles = div_up(cout, 64 * p.wm);
    p.ntiles = div_up(cin, 64 * p.wn);
    // ~3 workgroups per CU in total; a chunk is at least 256 rows and a multiple of the 32-row stage
    long long want = static_cast<long long>(kNumCU) * 3 / (p.mtiles * p.ntiles);
    if (want < 1) want = 1;
    long long rpc = (rows + want - 1) / want;
    if (rpc < 256) rpc = 256;
    rpc = (rpc + kGemmRowsPerStage - 1) / kGemmRowsPerStage * kGemmRowsPerStage;
    p.rows_per_chunk = rpc;
    p.chunks = static_cast<int>((rows + rpc - 1) / rpc);
    return p;
}

// Persistent tile loops: as many workgroups as are resident at once (LDS / VGPR bound per accumulator-tile count),
// times HF_GEMM_ROUNDS (default 2: whole rounds, and a tail that costs half as much when sampling pins a few CUs).
inline int resident_grid(int nt, long long ntiles)
{
    static const int per_cu[9] = { 0, 5, 4, 3, 3, 2, 2, 2, 2 };
    static const int rounds = HF_DIAG_INT("HF_GEMM_ROUNDS", 2) < 1 ? 1 : HF_DIAG_INT("HF_GEMM_ROUNDS", 2);
    long long g = static_cast<long long>(kNumCU) * per_cu[nt < 1 ? 1 : (nt > 8 ? 8 : nt)] * rounds;
    if (g > kBnMaxBlocks) g = kBnMaxBlocks;
    if (g > ntiles) g = ntiles;
    return static_cast<int>(g);
}

inline bool vec4_ok(const void *p, int ncols) { return ncols % 4 == 0 && reinterpret_cast<uintptr_t>(p) % 16 == 0; }

}  // namespace hf
