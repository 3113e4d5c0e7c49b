// lift_bwd.hip -- the first-layer backward of the lifting chain (gemm.hip, "The lifting chain of an X-Conv") in ONE sweep over dz1.
//
// hf_lift_elu_bn_bwd forms dy0 = dz1 W1 on the matrix cores twice: once for the BatchNorm-backward sums dbeta0 = sum dy0 and
// dgamma0 = sum dy0 xhat0, and again, those two known, for dz0 = a0 (dy0 - dbeta0/R - xhat0 dgamma0/R) elu'(z0) and dW0 = dz0^T x.
// dW0 is linear in the two sums.  With v = dy0[r][c], s = elu'(z0), xhat = (elu(z0) - mu_c) invstd_c and d = 0, 1, 2:
//   dW0[c][d] = a_c (A_d - (dbeta_c / R) B_d - (dgamma_c / R) C_d)
//   A_d = sum_r v (s x_d)      B_d = sum_r s x_d      C_d = sum_r xhat (s x_d)
// so one sweep that keeps eleven sums per channel (sum v, sum v xhat, A, B, C) replaces both, and a finalize kernel evaluates the
// formula in fp64 from the fp64 sums of the per-workgroup partials.
//
// Where B_d and C_d are summed: in the SAME epilogue, eleven sums per lane and column.  They do not depend on dz1 and could come
// from a pass over x alone (a lane per channel, as lift_stats_kernel), but that pass evaluates z0, the exponential and xhat for every
// (row, channel) a second time -- 25 VALU operations per element against the 12 that B and C add here, where z0, s and s x_d are
// already in registers -- and costs a launch that reads x again.  The compiled resource table decides whether the epilogue can carry
// them (profiles/lift_bwd_instantiations.md): NT = 1 .. 4 (c0 <= 128, every lifting layer of both stages) compile without spills
// or scratch below 256 VGPRs and with two workgroups' LDS in a CU; NT = 5 does not, so the entry stops at c0 = 128 and wider
// chains keep the two-pass entry.
//
// dbeta0 and dgamma0 keep the bits of the two-pass entry: the sweep is lift_linear_bwd_kernel<NT, 0>'s tile loop, staging, grid and
// epilogue row order with that kernel's own expressions for the first two sums, col_sums_store adds the lanes and waves in its one
// order, and the finalize adds the workgroups' partials in bn_reduce_channel's order (mlp.hip) for either of its two forms.
#include <stdint.h>

#include "hf_common.h"
#include "gemm_common.h"
#include "lift_common.h"

namespace hf {

constexpr int kSumV = 0, kSumVX = 1, kSumA = 2, kSumB = 5, kSumC = 8;   // rows of the partial-sum block, kLiftOnePassSums in all

// The scalar twin's staging load (kdim % 4 != 0, or dz1 / w1_t off a 16-byte boundary): load4_guarded<false> with every column index
// clamped instead of predicated.  The same values reach LDS; the address predicates that load4_guarded keeps in SGPR pairs across the
// tile loop do not exist, which is what keeps <2, false> and <4, false> free of SGPR spills.
__device__ __forceinline__ float4 load4_clamped(const float *__restrict__ base, long long row, long long row_end, int col, int ncols)
{
    const bool row_ok = row < row_end;
    const float *p = base + (row_ok ? row : 0) * ncols;
    const int last = ncols - 1;
    const float x = p[min(col, last)], y = p[min(col + 1, last)], z = p[min(col + 2, last)], w = p[min(col + 3, last)];
    float4 v;
    v.x = (row_ok && col < ncols) ? x : 0.f; v.y = (row_ok && col + 1 < ncols) ? y : 0.f;
    v.z = (row_ok && col + 2 < ncols) ? z : 0.f; v.w = (row_ok && col + 3 < ncols) ? w : 0.f;
    return v;
}

// VEC (kdim % 4 == 0, dz1 and w1_t 16-byte aligned) is a template argument here, not the run-time switch of lift_linear_bwd_kernel:
// with both load forms in one kernel the eleven sums do not fit (NT = 3 and 4 spill VGPRs, every NT spills SGPRs).  The scalar twin
// stages rows of W1^T past c0 as copies of row c0 - 1 instead of zeros: those accumulator columns are skipped by the epilogue
// and never stored, and the row predicates of the NT weight loads need not stay live.
template <int NT, bool VEC>
__global__ __launch_bounds__(kGemmThreads) __attribute__((amdgpu_waves_per_eu(2))) void lift_bwd_onepass_kernel(
    long long rows, int kdim, int c0, long long ntiles, const float *__restrict__ DZ, const float *__restrict__ WT,
    const float *__restrict__ x3, const float *__restrict__ w0, const float *__restrict__ mean0, const float *__restrict__ invstd0,
    float *__restrict__ partial)
{
    constexpr int NV = kLiftOnePassSums;
    __shared__ FwdLds<NT, NV> lds;
    const int t = threadIdx.x, lane = t & 63;
    // constants of this lane's output columns (channels of the first layer)
    float wx[NT], wy[NT], wz[NT], pmu[NT], pis[NT], acc_s[NT][NV];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const int col = nt * 32 + (lane & 31);
        const bool ok = col < c0;
        wx[nt] = ok ? w0[3 * col] : 0.f; wy[nt] = ok ? w0[3 * col + 1] : 0.f; wz[nt] = ok ? w0[3 * col + 2] : 0.f;
        pmu[nt] = ok ? mean0[col] : 0.f; pis[nt] = ok ? invstd0[col] : 0.f;
#pragma unroll
        for (int v = 0; v < NV; ++v) acc_s[nt][v] = 0.f;
    }
    const int k4 = fwd_k4(), srow = fwd_srow();
    float4 ar[4], br[NT];
    auto fetch = [&](long long r0, int kc) {
#pragma unroll
        for (int p = 0; p < 4; ++p)
            ar[p] = VEC ? load4_guarded<true>(DZ, r0 + srow + 32 * p, rows, kc + k4, kdim) : load4_clamped(DZ, r0 + srow + 32 * p, rows, kc + k4, kdim);
#pragma unroll
        for (int p = 0; p < NT; ++p)
            br[p] = VEC ? load4_guarded<true>(WT, srow + 32 * p, c0, kc + k4, kdim) : load4_clamped(WT, min(srow + 32 * p, c0 - 1), c0, kc + k4, kdim);
    };
    if (blockIdx.x < ntiles) fetch(static_cast<long long>(blockIdx.x) * kFwdRows, 0);
    for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const long long row0 = tile * kFwdRows;
        f32x16 acc[NT];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int g = 0; g < 16; ++g) acc[nt][g] = 0.f;
        for (int kc = 0; kc < kdim; kc += kFwdKC) {
#pragma unroll
            for (int p = 0; p < 4; ++p) *reinterpret_cast<float4 *>(&lds.As[(srow + 32 * p) * kFwdLS + k4]) = ar[p];
#pragma unroll
            for (int p = 0; p < NT; ++p) *reinterpret_cast<float4 *>(&lds.Bs[(srow + 32 * p) * kFwdLS + k4]) = br[p];
            __syncthreads();
            if (kc + kFwdKC < kdim) fetch(row0, kc + kFwdKC);
            else if (tile + gridDim.x < ntiles) fetch((tile + gridDim.x) * kFwdRows, 0);
            fwd_mfma_stage(lds, acc);
            __syncthreads();
        }
#pragma unroll
        for (int g = 0; g < 16; ++g) {
            const long long row = fwd_d_row(row0, g);
            if (row >= rows) continue;
            const float x0 = x3[3 * row], x1 = x3[3 * row + 1], x2 = x3[3 * row + 2];
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                if (nt * 32 + (lane & 31) >= c0) continue;
                const float v = acc[nt][g];
                const float z0 = lift_z(wx[nt], wy[nt], wz[nt], x0, x1, x2);
                const float xhat = (elu_hw(z0) - pmu[nt]) * pis[nt];
                acc_s[nt][kSumV] += v;
                acc_s[nt][kSumVX] += v * xhat;
                const float s = elu_hw_slope(z0);
                const float sx[3] = { s * x0, s * x1, s * x2 };
#pragma unroll
                for (int d = 0; d < 3; ++d) {
                    acc_s[nt][kSumA + d] += v * sx[d];
                    acc_s[nt][kSumB + d] += sx[d];
                    acc_s[nt][kSumC + d] += xhat * sx[d];
                }
            }
        }
    }
    col_sums_store(lds, acc_s, c0, partial);
}

// One workgroup per channel: the kLiftOnePassSums rows of the channel's partials are added over the workgroups in fp64, each in
// bn_reduce_channel's order for this nblk (mlp.hip) -- up to 256 workgroups a single wave walks a row (lane, lane + 64, ...) and folds
// its lanes by xor-shuffles (here wave w takes the rows w, w + 4, ...); above that all four waves walk it (t, t + 256, ...) and their
// sums meet in wave order.  dbeta0 and dgamma0 are rounded as bn_bwd_finalize_kernel rounds them; dW0 is evaluated in fp64 and rounded
// once.  No atomics: the same bits on every call.
__global__ __launch_bounds__(256) void lift_bwd_onepass_finalize_kernel(long long rows, int c0, int nblk, const float *__restrict__ partial,
                                                                       const float *__restrict__ gamma0, const float *__restrict__ invstd0,
                                                                       float *__restrict__ dgamma0, float *__restrict__ dbeta0,
                                                                       float *__restrict__ grad_w0_t)
{
    constexpr int NV = kLiftOnePassSums;
    __shared__ double wsum[NV][4];
    const int ch = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool wide = nblk > 256;   // bn_finalize_wide
    const int first = wide ? static_cast<int>(threadIdx.x) : lane, stride = wide ? 256 : 64;
    for (int v = wide ? 0 : wave; v < NV; v += wide ? 1 : 4) {
        const float *p = partial + (static_cast<size_t>(v) * c0 + ch) * kBnMaxBlocks;
        float val[8];   // nblk <= kBnMaxBlocks = 8 * 256: every load of the row is requested before the first add
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int k = first + u * stride;
            val[u] = k < nblk ? p[k] : 0.0f;
        }
        double a = 0.0;
#pragma unroll
        for (int u = 0; u < 8; ++u) a += static_cast<double>(val[u]);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) a += __shfl_xor(a, off);
        if (lane == 0) wsum[v][wide ? wave : 0] = a;
    }
    __syncthreads();
    if (threadIdx.x >= 3) return;
    double S[NV];
#pragma unroll
    for (int v = 0; v < NV; ++v) {
        double a = wsum[v][0];
        if (wide) {
#pragma unroll
            for (int w = 1; w < 4; ++w) a += wsum[v][w];
        }
        S[v] = a;
    }
    const int d = threadIdx.x;
    if (d == 0) {
        dbeta0[ch] = static_cast<float>(S[kSumV]);
        dgamma0[ch] = static_cast<float>(S[kSumVX]);
    }
    const double r = static_cast<double>(rows);
    const double a0 = static_cast<double>(gamma0[ch]) * static_cast<double>(invstd0[ch]);
    const double A = d == 0 ? S[kSumA] : (d == 1 ? S[kSumA + 1] : S[kSumA + 2]);
    const double B = d == 0 ? S[kSumB] : (d == 1 ? S[kSumB + 1] : S[kSumB + 2]);
    const double C = d == 0 ? S[kSumC] : (d == 1 ? S[kSumC + 1] : S[kSumC + 2]);
    grad_w0_t[static_cast<size_t>(d) * c0 + ch] = static_cast<float>(a0 * (A - (S[kSumV] / r) * B - (S[kSumVX] / r) * C));
}

int launch_lift_bwd_onepass(long long rows, int c1, int c0, const float *dz1, const float *w1_t, const float *x3, const float *w0,
                            const float *gamma0, const float *mean0, const float *invstd0, float *partial, float *grad_w0_t,
                            float *dgamma0, float *dbeta0, hipStream_t st)
{
    const long long ntiles = (rows + kFwdRows - 1) / kFwdRows;
    const int nt = div_up(c0, 32);
    const int nblk = resident_grid(nt, ntiles);
    const bool vec = vec4_ok(dz1, c1) && vec4_ok(w1_t, c1);
#define HF_LIFT_ONEPASS_V(N, V)                                                                                         \
    hipLaunchKernelGGL((lift_bwd_onepass_kernel<N, V>), dim3(nblk), dim3(kGemmThreads), 0, st, rows, c1, c0, ntiles, dz1, w1_t, x3, w0, \
                       mean0, invstd0, partial)
#define HF_LIFT_ONEPASS(N)                                                                                              \
    case N:                                                                                                             \
        if (vec) HF_LIFT_ONEPASS_V(N, true); else HF_LIFT_ONEPASS_V(N, false);                                          \
        break
    switch (nt) {
        HF_LIFT_ONEPASS(1); HF_LIFT_ONEPASS(2); HF_LIFT_ONEPASS(3); HF_LIFT_ONEPASS(4);
        default: return HF_EINVAL;
    }
#undef HF_LIFT_ONEPASS
#undef HF_LIFT_ONEPASS_V
    static_assert(kLiftOnePassMaxC0 == 4 * 32, "the instantiations above");
    hipLaunchKernelGGL(lift_bwd_onepass_finalize_kernel, dim3(c0), dim3(256), 0, st, rows, c0, nblk, partial, gamma0, invstd0, dgamma0,
                       dbeta0, grad_w0_t);
    return launch_status();
}

}  // namespace hf
