// gemm_common.h -- the tile machine shared by the MFMA GEMM sources (gemm.hip, fp_linear.hip): tile constants, the guarded
// staging load, and the launch plans that both the launchers and the workspace queries must agree on.
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

// forward tiles: Z = A W^T, a workgroup owns 128 rows and all Cout columns
constexpr int kFwdRows = 128;   // rows per workgroup tile
constexpr int kFwdKC = 32;      // input channels per LDS stage
constexpr int kFwdLS = kFwdKC + 4;  // LDS row stride (keeps float4 stores aligned; 2-way read conflicts are noise here)

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
