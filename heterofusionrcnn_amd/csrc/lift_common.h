// lift_common.h -- what the lifting-chain kernels of gemm.hip and lift_bwd.hip share: the first layer's constants (LiftTab), the one
// expression that forms z0 (lift_z) and the normalised first-layer output (lift_y), so that the forward statistics, the operand of the
// second GEMM, the weight gradient and every backward pass see the same bits; and the launcher that lift_bwd.hip exports to the entry
// point in gemm.hip.
#pragma once
#include "hf_common.h"

namespace hf {

constexpr int kLiftMaxC = 256;
struct LiftTab {
    float wx[kLiftMaxC], wy[kLiftMaxC], wz[kLiftMaxC], a[kLiftMaxC], mu[kLiftMaxC], be[kLiftMaxC], is[kLiftMaxC];
};

__device__ __forceinline__ void lift_tab_load(LiftTab &T, int c, const float *__restrict__ w0, const float *__restrict__ gamma,
                                              const float *__restrict__ beta, const float *__restrict__ mean,
                                              const float *__restrict__ invstd)
{
    for (int k = threadIdx.x; k < c; k += blockDim.x) {
        T.wx[k] = w0[3 * k];
        T.wy[k] = w0[3 * k + 1];
        T.wz[k] = w0[3 * k + 2];
        T.a[k] = gamma[k] * invstd[k];
        T.mu[k] = mean[k];
        T.be[k] = beta[k];
        T.is[k] = invstd[k];
    }
}
__device__ __forceinline__ float lift_z(float wx, float wy, float wz, float x0, float x1, float x2) { return (x0 * wx + x1 * wy) + x2 * wz; }
// the first layer's ELU is evaluated five times per element instead of once, and expm1f (~30 instructions) made the lift
// kernels VALU-bound (the forward wrote its 268 MB in 119 us): elu_hw, exp(x) - 1 on the hardware exponential
__device__ __forceinline__ float lift_y(const LiftTab &T, int k, float x0, float x1, float x2)
{
    return T.a[k] * (elu_hw(lift_z(T.wx[k], T.wy[k], T.wz[k], x0, x1, x2)) - T.mu[k]) + T.be[k];
}
// the three coordinates of row `row`, zero outside [0, row_end)
__device__ __forceinline__ void lift_load_x(const float *__restrict__ x3, long long row, long long row_end, float (&x)[3])
{
    const bool ok = row < row_end;
    const float *px = x3 + (ok ? row : 0) * 3;
    const float a = px[0], b = px[1], c = px[2];
    x[0] = ok ? a : 0.f; x[1] = ok ? b : 0.f; x[2] = ok ? c : 0.f;
}
// y0 of channels k .. k+3 of a row with coordinates x; zero outside the matrix
__device__ __forceinline__ float4 lift_y4(const LiftTab &T, int k, int c0, bool rin, const float (&x)[3])
{
    float4 v;
    v.x = (rin && k < c0) ? lift_y(T, k, x[0], x[1], x[2]) : 0.f;
    v.y = (rin && k + 1 < c0) ? lift_y(T, k + 1, x[0], x[1], x[2]) : 0.f;
    v.z = (rin && k + 2 < c0) ? lift_y(T, k + 2, x[0], x[1], x[2]) : 0.f;
    v.w = (rin && k + 3 < c0) ? lift_y(T, k + 3, x[0], x[1], x[2]) : 0.f;
    return v;
}

// lift_bwd.hip: the first layer's backward in ONE sweep over dz1 (dgamma0, dbeta0, grad_w0_t).  kLiftOnePassSums per-workgroup
// column sums per channel go through `partial` (kLiftOnePassSums * c0 * kBnMaxBlocks floats).  c0 <= kLiftOnePassMaxC0, checked by the caller.
constexpr int kLiftOnePassSums = 11;
constexpr int kLiftOnePassMaxC0 = 128;
int launch_lift_bwd_onepass(long long rows, int c1, int c0, const float *dz1, const float *w1_t, const float *x3, const float *w0,
                            const float *gamma0, const float *mean0, const float *invstd0, float *partial, float *grad_w0_t,
                            float *dgamma0, float *dbeta0, hipStream_t st);

}  // namespace hf
