// xconv_bn.hip -- the gather-mode X-Conv kernels of xconv.hip with the lifting branch's last BatchNorm folded in.
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
// code of xconv_dw_fwd_kernel / xconv_dw_bwd_fw_kernel / xconv_dw_bwd_x_kernel with GATHER = true.  out, grad_x, grad_f, grad_wd and
// grad_fts are therefore the same bits as hf_bn_relu_fwd_eval + hf_xconv_depthwise_gather[_grad] give; dgamma / dbeta are summed in
// another order than bn_bwd_reduce_kernel's (per lane over its rows, the four waves in wave order, the blocks in double) and agree
// to fp32 rounding.  No atomics: the same bits on every call.
#include "xconv_common.h"

namespace hf {

// forward: xconv_dw_fwd_kernel<K, M, true, V2> with the lifted pairs normalised on load
template <int K, int M, bool V2>
__global__ __launch_bounds__(kXcThreads) void xconv_bn_fwd_kernel(long long rows, int c, int c0, int rows_per_block,
                                                                 const float *__restrict__ x, const float *__restrict__ z1,
                                                                 const float *__restrict__ gamma, const float *__restrict__ beta,
                                                                 const float *__restrict__ mean, const float *__restrict__ invstd,
                                                                 const float *__restrict__ fts, const int *__restrict__ idx, int n_src,
                                                                 int rows_per_cloud, const float *__restrict__ wd, float *__restrict__ out)
{
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6));
    const int ch = blockIdx.y * 128 + 2 * lane;
    const XcPair src = xc_pair(ch, c, c0, z1, fts, true);
    const int cw = src.live ? ch : (c - 1) & ~1;
    f2 w[K][M];
#pragma unroll
    for (int k = 0; k < K; ++k)
#pragma unroll
        for (int m = 0; m < M; ++m) w[k][m] = f2{wd[(static_cast<size_t>(k) * c + cw) * M + m], wd[(static_cast<size_t>(k) * c + cw + src.hi) * M + m]};
    // the pair's BatchNorm constants, loaded once like w (c0 is even: a lifted pair lies below c0 as a whole); a gathered lane
    // reads channel 0's, computes with them and keeps the raw value by select
    const int cb = src.gathered ? 0 : cw;
    const bool some_lifted = static_cast<int>(blockIdx.y) * 128 < c0;   // this block column holds lifted channels
    const f2 ba = f2{gamma[cb] * invstd[cb], gamma[cb + 1] * invstd[cb + 1]};
    const f2 bmu = f2{mean[cb], mean[cb + 1]}, bb = f2{beta[cb], beta[cb + 1]};
    const unsigned lstride = c0, c1 = c - c0;
    const long long r0 = static_cast<long long>(blockIdx.x) * rows_per_block;
    const long long r1 = r0 + rows_per_block < rows ? r0 + rows_per_block : rows;
    __shared__ float xs[kXcThreads / 64][kXcRows][K * K];
    XcCloud cl = xc_cloud(r0, rows_per_cloud, n_src);
    for (long long rb = r0 + wave; rb < r1; rb += 4 * kXcRows) {
        f2 fv[kXcRows][K];
        long long rr[kXcRows];
#pragma unroll
        for (int i = 0; i < kXcRows; ++i) rr[i] = rb + 4 * i < r1 ? rb + 4 * i : r1 - 1;
        XcXRows<K> xrow;
        xrow.load(x, rr, lane);
#pragma unroll
        for (int i = 0; i < kXcRows; ++i) {
            const unsigned tb = xc_tbase(cl, rr[i], rows_per_cloud, n_src);
            xc_gather_row<K, true, V2>(src, rr[i], tb, idx, lstride, c1, fv[i]);
        }
        xrow.stage(xs[wave], lane);
#pragma unroll
        for (int i = 0; i < kXcRows; ++i) {
            if (rb + 4 * i >= r1) break;
            if (some_lifted) {   // uniform over the block: the columns past the split (most of them) pay nothing
#pragma unroll
                for (int j = 0; j < K; ++j) {
                    const f2 z = fv[i][j];
                    const f2 h = ba * (f2{elu_stream(z.x), elu_stream(z.y)} - bmu) + bb;
                    fv[i][j] = src.gathered ? z : h;
                }
            }
            const float *xr = xs[wave][i];
            f2 o[M];
#pragma unroll
            for (int m = 0; m < M; ++m) o[m] = f2{0.f, 0.f};
#pragma unroll
            for (int k = 0; k < K; ++k) {
                f2 t = xr[k * K] * fv[i][0];
#pragma unroll
                for (int j = 1; j < K; ++j) t = t + xr[k * K + j] * fv[i][j];
#pragma unroll
                for (int m = 0; m < M; ++m) o[m] = o[m] + t * w[k][m];
            }
            if (src.live) st_pair_m<M, V2>(out + static_cast<size_t>(rr[i] * c + ch) * M, src.hi_live, o);
        }
    }
}

// gradients w.r.t. F_delta and Wd: xconv_dw_bwd_fw_kernel<K, M, true> with the lifted values normalised on load, plus the two
// BatchNorm-backward sums of the lifted channels (bn_bwd_reduce_kernel's expressions on the gradient this kernel stores): a lane owns
// one channel over all its rows, as it does for the Wd gradient; the four waves meet in LDS in wave order and the block writes
// bn_partial[blockIdx.x][0][c0] = sum gf, bn_partial[blockIdx.x][1][c0] = sum gf * xhat (xconv_bn_finalize_kernel adds the blocks)
// amdgpu_waves_per_eu(4): the grid is four blocks per CU (xdw_bwd_grid), one wave of each per SIMD; with the two sums carried
// through the row loop the scheduler otherwise trades that residency for up to 190 VGPRs (two or three waves per SIMD); held to
// 128 the kernels take 96 / 114 / 124 at M = 1 / 2 / 4, nothing spilled
template <int K, int M>
__global__ __launch_bounds__(kXcThreads) __attribute__((amdgpu_waves_per_eu(4))) void xconv_bn_bwd_fw_kernel(long long rows, int c, int c0, int rows_per_block,
                                                                    const float *__restrict__ x, const float *__restrict__ z1,
                                                                    const float *__restrict__ gamma, const float *__restrict__ beta,
                                                                    const float *__restrict__ mean, const float *__restrict__ invstd,
                                                                    const float *__restrict__ fts, const int *__restrict__ idx, int n_src,
                                                                    int rows_per_cloud, const float *__restrict__ wd,
                                                                    const float *__restrict__ grad_out, float *__restrict__ grad_f,
                                                                    float *__restrict__ grad_gathered, float *__restrict__ grad_wd,
                                                                    float *__restrict__ wd_partial, float *__restrict__ bn_partial)
{
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6));
    const int ch = blockIdx.y * 64 + lane;
    const bool live = ch < c;
    const XcSource src = xc_source(live ? ch : blockIdx.y * 64, c, c0, z1, fts, idx);
    if (src.gathered && !grad_wd && !grad_gathered) return;   // nothing of this chunk is asked for (no partial to write either)
    const bool lifted = static_cast<int>(blockIdx.y) * 64 < c0;   // = !src.gathered, uniform over the block; every lane of a lifted chunk is live
    const int cb = lifted ? ch : 0;
    const float bis = invstd[cb], ba = gamma[cb] * bis, bmu = mean[cb], bb = beta[cb];
    float s1 = 0.f, s2 = 0.f;
    float w[K][M], gw[K][M];
#pragma unroll
    for (int k = 0; k < K; ++k)
#pragma unroll
        for (int m = 0; m < M; ++m) { w[k][m] = live ? wd[(static_cast<size_t>(k) * c + ch) * M + m] : 0.f; gw[k][m] = 0.f; }
    const long long r0 = static_cast<long long>(blockIdx.x) * rows_per_block;
    const long long r1 = r0 + rows_per_block < rows ? r0 + rows_per_block : rows;
    for (long long r = r0 + wave; r < r1; r += kXcThreads / 64) {
        const float *xr = x + r * (K * K);
        float fv[K], xv[K], g[M], gfx[K];
        const long long tbase = src.gathered ? static_cast<long long>(static_cast<unsigned>(r) / static_cast<unsigned>(rows_per_cloud)) * n_src : 0;
#pragma unroll
        for (int j = 0; j < K; ++j) {
            const long long srow = src.gathered ? tbase + idx[r * K + j] : r * K + j;
            fv[j] = live ? src.base[srow * src.stride] : 0.f;
            xv[j] = 0.f;
        }
        if (lifted) {   // a uniform branch behind the loads: z1 -> F_delta, elu(z1) kept for the sums below
#pragma unroll
            for (int j = 0; j < K; ++j) {
                xv[j] = elu_stream(fv[j]);
                fv[j] = ba * (xv[j] - bmu) + bb;
            }
        }
        load_m<M>(grad_out, static_cast<size_t>(r * c + (live ? ch : 0)) * M, g);
        if (!live) {
#pragma unroll
            for (int m = 0; m < M; ++m) g[m] = 0.f;
        }
#pragma unroll
        for (int k = 0; k < K; ++k) {
            float a = 0.f;
#pragma unroll
            for (int m = 0; m < M; ++m) a = a + g[m] * w[k][m];          // = hf_depthwise_k_grad's dx
            gfx[k] = a;
            float t = xr[k * K] * fv[0];                                  // F_X recomputed
#pragma unroll
            for (int j = 1; j < K; ++j) t = t + xr[k * K + j] * fv[j];
#pragma unroll
            for (int m = 0; m < M; ++m) gw[k][m] = gw[k][m] + t * g[m];   // = hf_depthwise_k_grad's dw
        }
        float *gdst = src.gathered ? (grad_gathered ? grad_gathered + (ch - c0) : nullptr) : (grad_f ? grad_f + ch : nullptr);
        if (live && gdst) {
            float ga[K];
#pragma unroll
            for (int j = 0; j < K; ++j) {
                float a = xr[j] * gfx[0];                                  // = hf_xconv_apply_grad's dF (X transposed)
#pragma unroll
                for (int k = 1; k < K; ++k) a = a + xr[k * K + j] * gfx[k];
                gdst[(r * K + j) * src.stride] = a;
                ga[j] = a;
            }
            if (lifted) {   // = bn_bwd_reduce_kernel's sums with dh = the value just stored (behind the stores: inside their loop the sums cost 40 VGPRs)
#pragma unroll
                for (int j = 0; j < K; ++j) { s1 += ga[j]; s2 += ga[j] * ((xv[j] - bmu) * bis); }
            }
        }
    }
    __shared__ float red[K * M][64];
    if (lifted && grad_f) {
        // the waves take turns, wave 0 first, on two rows of `red` (a fixed order of adds); the Wd reduction below reuses them
        for (int wv = 0; wv < kXcThreads / 64; ++wv) {
            if (wave == wv) {
                red[0][lane] = wv == 0 ? s1 : red[0][lane] + s1;
                red[1][lane] = wv == 0 ? s2 : red[1][lane] + s2;
            }
            __syncthreads();
        }
        if (wave == 0) {   // the slots it reads are its own: the first writer below is this same thread
            float *mine = bn_partial + static_cast<size_t>(blockIdx.x) * 2 * c0;
            mine[ch] = red[0][lane];
            mine[c0 + ch] = red[1][lane];
        }
    }
    if (grad_wd) {
        // as xconv_dw_bwd_fw_kernel: the waves take turns, wave 0 first; the row chunks' sums go to wd_partial[row chunk][K*c*M] and
        // are added in a fixed order by a second kernel
        for (int wv = 0; wv < kXcThreads / 64; ++wv) {
            if (wave == wv && live) {
#pragma unroll
                for (int k = 0; k < K; ++k)
#pragma unroll
                    for (int m = 0; m < M; ++m) red[k * M + m][lane] = wv == 0 ? gw[k][m] : red[k * M + m][lane] + gw[k][m];
            }
            __syncthreads();
        }
        float *mine = wd_partial + static_cast<size_t>(blockIdx.x) * K * c * M;
        for (int i = threadIdx.x; i < K * M * 64; i += kXcThreads) {
            const int km = i >> 6, c2 = blockIdx.y * 64 + (i & 63);
            if (c2 < c) mine[(static_cast<size_t>(km / M) * c + c2) * M + km % M] = red[km][i & 63];
        }
    }
}

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
    hipLaunchKernelGGL((xconv_bn_fwd_kernel<KK, MM, V>), grid, dim3(kXcThreads), 0, st, rows, c, c0, rpb, x, z1, gamma, beta, mean, invstd, fts, idx, n_src, rows_per_cloud, wd, out);
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
    const long long rows = static_cast<long long>(b) * rows_per_cloud, src_rows = static_cast<long long>(b) * n_src;
    const int c = c0 + c1;
    if (rows == 0) {   // an empty batch: every gradient that is asked for is zero
        int rc = HF_OK;
        if (grad_wd) rc = hip_status(hipMemsetAsync(grad_wd, 0, sizeof(float) * static_cast<size_t>(k) * c * m, st));
        if (rc == HF_OK && grad_fts && src_rows > 0) rc = hip_status(hipMemsetAsync(grad_fts, 0, sizeof(float) * static_cast<size_t>(src_rows) * c1, st));
        if (rc == HF_OK && grad_f) rc = hip_status(hipMemsetAsync(dgamma, 0, sizeof(float) * c0, st));
        if (rc == HF_OK && grad_f) rc = hip_status(hipMemsetAsync(dbeta, 0, sizeof(float) * c0, st));
        return rc;
    }
    if (!workspace || workspace_bytes < hf_xconv_depthwise_gather_bn_grad_workspace(b, rows_per_cloud, k, c0, c1, m)) return HF_EWORKSPACE;
    // the table's gradient: rebuilt per table row, or staged in the workspace and summed per table row, as xdw_fts_direct picks
    // for the shape (hf_xconv_depthwise_gather_grad with a workspace: the same routes, the same bits)
    const bool want_fts = grad_fts != nullptr;
    const bool direct = want_fts && xdw_fts_direct(rows, n_src, rows_per_cloud, k, c1, m);
    unsigned char *ws = static_cast<unsigned char *>(workspace);
    float *gathered = (want_fts && !direct) ? static_cast<float *>(workspace) : nullptr;
    float *wd_partial = grad_wd ? reinterpret_cast<float *>(ws + xdw_gathered_bytes(b, rows_per_cloud, k, c1)) : nullptr;
    float *bn_partial = reinterpret_cast<float *>(ws + xbn_base_bytes(b, rows_per_cloud, k, c0, c1, m));
    if (grad_f || grad_wd || gathered) {
        dim3 grid;
        int rpb;
        xdw_bwd_grid(rows, c, grid, rpb);
#define HF_XBN_BFW(KK, MM)                                                                                             \
        hipLaunchKernelGGL((xconv_bn_bwd_fw_kernel<KK, MM>), grid, dim3(kXcThreads), 0, st, rows, c, c0, rpb, x, z1, gamma, beta, mean, invstd, fts, idx, n_src, rows_per_cloud, wd, grad_out, grad_f, gathered, grad_wd, wd_partial, bn_partial);
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
    if (gathered) return hf_group_point_grad_gather(b, n_src, c1, rows_per_cloud, k, c1, 0, gathered, offsets, entries, grad_fts, stream);
    if (direct) return xdw_table_grad(src_rows, n_src, rows_per_cloud, k, c, c0, m, x, wd, grad_out, offsets, entries, grad_fts, st);
    return HF_OK;
}
