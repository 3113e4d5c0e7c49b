// xconv_bn.hip -- the gather-mode X-Conv kernels with the lifting branch's last BatchNorm folded in: the kernel templates of
// xconv_common.h instantiated with BN on (xconv_dw_fwd_kernel<K, M, true, V2, true>, xconv_dw_bwd_fw_kernel<K, M, true, true>, and
// xc_bwd_x_body behind xconv_bn_bwd_x_kernel), plus the kernel that finishes the two BatchNorm sums.
//
// On the gather route F_* = [F_delta | fts[idx]] and F_delta = BN1(elu(z1)) is an elementwise function of the lifting chain's
// pre-activation z1 (rows x K x c0) and four per-channel constants.  The kernels of xconv.hip read F_delta from memory: one
// pass (bn_apply_kernel of mlp.hip) writes it, and in the backward one more pass (bn_bwd_reduce_kernel) reads z1 and the gradient
// of F_delta back only to form two sums per channel.  Here the three kernels that read the lifted half take z1 and
// (gamma, beta, mean, invstd) instead and rebuild F_delta on load, and the kernel that stores the gradient of F_delta sums
// dbeta = sum gf and dgamma = sum gf * xhat from the values it holds: neither pass exists, F_delta is never written.
//
// The arithmetic is that of the two routes it replaces, element for element: the normalisation is bn_apply_kernel's
// a = gamma * invstd; h = a * (elu_stream(z) - mean) + beta (multiply, then add: -ffp-contract=off), everything behind it is the
// very code xconv.hip instantiates with GATHER = true and BN off.  out, grad_x, grad_f, grad_wd and
// grad_fts are therefore the same bits as hf_bn_relu_fwd_eval + hf_xconv_depthwise_gather[_grad] give; dgamma / dbeta are summed in
// another order than bn_bwd_reduce_kernel's (per lane over its rows, the four waves in wave order, the blocks in double) and agree
// to fp32 rounding.  No atomics: the same bits on every call.
#include "xconv_common.h"

namespace hf {

// dbeta[ch] = sum over the blocks of bn_partial[blk][0][ch], dgamma[ch] = ... [1][ch]: one workgroup per channel, each thread adds
// its blocks (t, t + 256, ...) in double, then the lanes and the four waves meet in a fixed order (as bn_bwd_finalize_kernel's
// wide form)
__global__ __launch_bounds__(kXcThreads) void xconv_bn_finalize_kernel(int c0, int nblk, const float *__restrict__ bn_partial,
                                                                      float *__restrict__ dgamma, float *__restrict__ dbeta)
{
    __shared__ double cross[2][kXcThreads / 64];
    const int ch = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double a = 0.0, b = 0.0;
    for (int i = threadIdx.x; i < nblk; i += kXcThreads) {
        a += static_cast<double>(bn_partial[static_cast<size_t>(i) * 2 * c0 + ch]);
        b += static_cast<double>(bn_partial[static_cast<size_t>(i) * 2 * c0 + c0 + ch]);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { a += __shfl_xor(a, off); b += __shfl_xor(b, off); }
    if (lane == 0) { cross[0][wave] = a; cross[1][wave] = b; }
    __syncthreads();
    if (threadIdx.x == 0) {
        a = cross[0][0]; b = cross[1][0];
#pragma unroll
        for (int w = 1; w < kXcThreads / 64; ++w) { a += cross[0][w]; b += cross[1][w]; }
        dbeta[ch] = static_cast<float>(a);
        dgamma[ch] = static_cast<float>(b);
    }
}

// gradient w.r.t. X: xconv_dw_bwd_x_kernel<K, M, true> with the lifted values normalised on load (xc_bwd_x_body with BN on)
template <int K, int M>
__global__ __launch_bounds__(kXcThreads) void xconv_bn_bwd_x_kernel(long long rows, int c, int c0, const float *__restrict__ z1,
                                                                   const float *__restrict__ gamma, const float *__restrict__ beta,
                                                                   const float *__restrict__ mean, const float *__restrict__ invstd,
                                                                   const float *__restrict__ fts, const int *__restrict__ idx, int n_src,
                                                                   int rows_per_cloud, const float *__restrict__ wd,
                                                                   const float *__restrict__ grad_out, float *__restrict__ grad_x)
{
    extern __shared__ float lds[];
    xc_bwd_x_body<K, M, true, true>(rows, c, c0, z1, gamma, beta, mean, invstd, fts, idx, n_src, rows_per_cloud, wd, grad_out, grad_x, lds);
}

}  // namespace hf

using namespace hf;

// (k, m) of the gather layers of the shipped PointCNN configurations: the encoder and decoder X-Convs of rpn_multiclass.config
#define HF_XBN_DISPATCH(CALL)                                                                                          \
    if (k == 8 && m == 1) { CALL(8, 1) } else if (k == 8 && m == 2) { CALL(8, 2) } else if (k == 8 && m == 4) { CALL(8, 4) }      \
    else return HF_EINVAL;

static bool xbn_km_ok(int k, int m) { return k == 8 && (m == 1 || m == 2 || m == 4); }

static bool xbn_shape_ok(int b, int n_src, int rows_per_cloud, int k, int c0, int c1, int m)
{
    if (b < 0 || n_src <= 0 || rows_per_cloud < 0 || c0 <= 0 || c0 % 64 != 0 || c1 <= 0 || !xbn_km_ok(k, m)) return false;
    const long long rows = static_cast<long long>(b) * rows_per_cloud;
    return rows <= 0x7fffffffll && xdw_offsets_fit(rows, k, c0 + c1, static_cast<long long>(b) * n_src);
}

static size_t xbn_align(size_t bytes) { return (bytes + 255) & ~static_cast<size_t>(255); }

HF_API int hf_xconv_depthwise_gather_bn(int b, int n_src, int rows_per_cloud, int k, int c0, int c1, int m, const float *x,
                                        const float *z1, const float *gamma, const float *beta, const float *mean,
                                        const float *invstd, const float *fts, const int *idx, const float *wd, float *out,
                                        hf_stream_t stream)
{
    if (!xbn_shape_ok(b, n_src, rows_per_cloud, k, c0, c1, m)) return HF_EINVAL;
    const long long rows = static_cast<long long>(b) * rows_per_cloud;
    if (rows == 0) return HF_OK;
    if (!x || !z1 || !gamma || !beta || !mean || !invstd || !fts || !idx || !wd || !out) return HF_EINVAL;
    const int c = c0 + c1;
    dim3 grid;
    int rpb;
    xdw_pair_grid(rows, c, grid, rpb, 8);
    const bool v2 = xdw_v2(c, {z1, fts, out});
    hipStream_t st = as_stream(stream);
#define HF_XBN_FWD_V(KK, MM, V)                                                                                        \
    hipLaunchKernelGGL((xconv_dw_fwd_kernel<KK, MM, true, V, true>), grid, dim3(kXcThreads), 0, st, rows, c, c0, rpb, x, z1, gamma, beta, mean, invstd, fts, idx, n_src, rows_per_cloud, wd, out);
#define HF_XBN_FWD(KK, MM) if (v2) { HF_XBN_FWD_V(KK, MM, true) } else { HF_XBN_FWD_V(KK, MM, false) }
    HF_XBN_DISPATCH(HF_XBN_FWD)
#undef HF_XBN_FWD
#undef HF_XBN_FWD_V
    return launch_status();
}

// [hf_xconv_depthwise_gather_grad_workspace's two regions][BatchNorm partial sums: row chunks x 2 x c0]
static size_t xbn_base_bytes(int b, int rows_per_cloud, int k, int c0, int c1, int m)
{
    return xbn_align(hf_xconv_depthwise_gather_grad_workspace(b, rows_per_cloud, k, c0, c1, m));
}

HF_API size_t hf_xconv_depthwise_gather_bn_grad_workspace(int b, int rows_per_cloud, int k, int c0, int c1, int m)
{
    if (b <= 0 || rows_per_cloud <= 0 || k <= 0 || c0 <= 0 || c1 <= 0 || m <= 0) return 0;
    dim3 grid;
    int rpb;
    xdw_bwd_grid(static_cast<long long>(b) * rows_per_cloud, c0 + c1, grid, rpb);
    return xbn_base_bytes(b, rows_per_cloud, k, c0, c1, m) + sizeof(float) * static_cast<size_t>(grid.x) * 2 * c0;
}

HF_API int hf_xconv_depthwise_gather_bn_grad(int b, int n_src, int rows_per_cloud, int k, int c0, int c1, int m, const float *x,
                                             const float *z1, const float *gamma, const float *beta, const float *mean,
                                             const float *invstd, const float *fts, const int *idx, const float *wd,
                                             const float *grad_out, const int *offsets, const int *entries, float *grad_x,
                                             float *grad_f, float *grad_fts, float *grad_wd, float *dgamma, float *dbeta,
                                             void *workspace, size_t workspace_bytes, hf_stream_t stream)
{
    if (!xbn_shape_ok(b, n_src, rows_per_cloud, k, c0, c1, m) || !x || !z1 || !gamma || !beta || !mean || !invstd || !fts || !idx || !wd ||
        !grad_out || (!grad_x && !grad_f && !grad_fts && !grad_wd))
        return HF_EINVAL;
    if ((grad_fts && (!offsets || !entries)) || (grad_f && (!dgamma || !dbeta))) return HF_EINVAL;
    hipStream_t st = as_stream(stream);
    const long long rows = static_cast<long long>(b) * rows_per_cloud;
    const int c = c0 + c1;
    if (rows == 0) {   // an empty batch: every gradient that is asked for is zero
        int rc = xdw_grad_empty(b, n_src, k, c0, c1, m, grad_fts, grad_wd, st);
        if (rc == HF_OK && grad_f) rc = hip_status(hipMemsetAsync(dgamma, 0, sizeof(float) * c0, st));
        if (rc == HF_OK && grad_f) rc = hip_status(hipMemsetAsync(dbeta, 0, sizeof(float) * c0, st));
        return rc;
    }
    if (!workspace || workspace_bytes < hf_xconv_depthwise_gather_bn_grad_workspace(b, rows_per_cloud, k, c0, c1, m)) return HF_EWORKSPACE;
    // hf_xconv_depthwise_gather_grad's plan with a workspace: the same routes to the table's gradient, the same bits
    const XdwGradPlan plan = xdw_grad_plan(b, n_src, rows_per_cloud, k, c1, m, grad_fts, workspace);
    float *gathered = plan.gathered, *wd_partial = plan.wd_partial;
    float *bn_partial = reinterpret_cast<float *>(static_cast<unsigned char *>(workspace) + xbn_base_bytes(b, rows_per_cloud, k, c0, c1, m));
    if (grad_f || grad_wd || gathered) {
        dim3 grid;
        int rpb;
        xdw_bwd_grid(rows, c, grid, rpb);
#define HF_XBN_BFW(KK, MM)                                                                                             \
        hipLaunchKernelGGL((xconv_dw_bwd_fw_kernel<KK, MM, true, true>), grid, dim3(kXcThreads), 0, st, rows, c, c0, rpb, x, z1, gamma, beta, mean, invstd, fts, idx, n_src, rows_per_cloud, wd, grad_out, grad_f, gathered, grad_wd, wd_partial, bn_partial);
        HF_XBN_DISPATCH(HF_XBN_BFW)
#undef HF_XBN_BFW
        if (grad_wd) launch_partial_reduce(k * c * m, static_cast<int>(grid.x), wd_partial, grad_wd, st);
        if (grad_f) hipLaunchKernelGGL(xconv_bn_finalize_kernel, dim3(c0), dim3(kXcThreads), 0, st, c0, static_cast<int>(grid.x), bn_partial, dgamma, dbeta);
        const int rc = launch_status();
        if (rc != HF_OK) return rc;
    }
    if (grad_x) {
        const size_t lds = xc_bwd_x_lds_bytes(c, c0, k * m);   // the staged Wd and BatchNorm constants
#define HF_XBN_BX(KK, MM)                                                                                              \
        hipLaunchKernelGGL((xconv_bn_bwd_x_kernel<KK, MM>), dim3(grid_for(rows, kXcThreads / 64)), dim3(kXcThreads), lds, st, rows, c, c0, z1, gamma, beta, mean, invstd, fts, idx, n_src, rows_per_cloud, wd, grad_out, grad_x);
        HF_XBN_DISPATCH(HF_XBN_BX)
#undef HF_XBN_BX
        const int rc = launch_status();
        if (rc != HF_OK) return rc;
    }
    return xdw_grad_table(plan, b, n_src, rows_per_cloud, k, c0, c1, m, x, wd, grad_out, offsets, entries, grad_fts, stream);
}
