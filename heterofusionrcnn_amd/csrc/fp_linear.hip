// fp_linear.hip -- the FIRST layer of a feature-propagation MLP on three_nn rows read in place, for gfx950.
//
// pointnet_fp_module (hf/core/feature_extractors/pointnet_util.py:303-329) interpolates points2 at the three nearest
// known points of every dense point, concatenates the skip features points1 behind the result and hands that (B, N, C2 + C1)
// tensor to the first tf_util.conv2d([1,1]).  Here the operand rows of that layer's GEMM and of its weight gradient are
// assembled from (points2, idx, weight3, points1) while they are staged for the MFMA tiles, so the concatenated tensor is
// neither written nor read back (the FP twin of the gathering first layer of a set abstraction).
//
// Operand row r (cloud = r / rows_per_cloud), the column order of hf_three_interpolate_concat, so the layer's weight is used
// as it is (zero-padded to cin columns):
//   [ interp(0 .. c2-1) | skip(0 .. c1-1) | zeros up to cin = round_up(c2 + c1, 4) ]
//   interp(j) = w[r][0] * P[cloud, idx[r][0], j] + w[r][1] * P[cloud, idx[r][1], j] + w[r][2] * P[cloud, idx[r][2], j]
// summed left to right without contraction: the bits of three_interpolate_concat_kernel (interpolate.hip).
//
// The tile machine is that of gemm.hip, shared through gemm_common.h (fwd_mfma_stage, col_sums_store, wgrad_tile_loop):
// v_mfma_f32_32x32x2_f32, 128-row forward tiles of 32 input channels per LDS stage on a persistent grid with the BatchNorm
// statistics taken from the accumulators; the weight gradient as per-chunk partial tiles summed in a fixed order.  This file is
// the A-operand loader (InterpSrc), the two kernels that hand it to the machine, and their launchers.
#include <math.h>
#include <stdint.h>

#include "hf_common.h"
#include "gemm_common.h"

namespace hf {

struct InterpSrc {
    const float *points2;       // (B, m, c2)
    const int *idx;             // (rows, 3) three_nn indices into the row's own cloud
    const float *w3;            // (rows, 3) interpolation weights
    const float *skip;          // (rows, c1); unused when c1 == 0
    int c2, c1, m;
    unsigned rows_per_cloud;
    bool skip_vec;              // c2 % 4 == 0, c1 % 4 == 0 and `skip` 16-byte aligned: a chunk of the skip part is one 16-byte load
};

// the three rows of points2 (flattened over clouds) that operand row `row` interpolates; rows outside the matrix name row 0.
// An index outside [0, m) is clamped into the cloud, so a corrupt table cannot send a load outside points2.
__device__ __forceinline__ void interp_row_idx(const InterpSrc &s, long long row, long long row_end, unsigned (&src)[3])
{
    const long long r = row < row_end ? row : 0;
    const unsigned base = static_cast<unsigned>(r) / s.rows_per_cloud * static_cast<unsigned>(s.m);   // rows < 2^32, clouds * m < 2^31
    const int *k = s.idx + r * 3;
    const int k0 = k[0], k1 = k[1], k2 = k[2];
    src[0] = base + static_cast<unsigned>(min(max(k0, 0), s.m - 1));
    src[1] = base + static_cast<unsigned>(min(max(k1, 0), s.m - 1));
    src[2] = base + static_cast<unsigned>(min(max(k2, 0), s.m - 1));
}

__device__ __forceinline__ void interp_row_w(const InterpSrc &s, long long row, long long row_end, float (&w)[3])
{
    const float *p = s.w3 + (row < row_end ? row : 0) * 3;
    w[0] = p[0]; w[1] = p[1]; w[2] = p[2];
}

// Loads behind operand columns col .. col+3 (col a multiple of 4) of row `row`: the three gathered chunks of points2, or the
// chunk of the skip row in d[0].  Nothing is multiplied here: the loads stay in flight until interp_combine.
// VEC: c2 % 4 == 0 and points2 16-byte aligned, so a chunk lies on one side of the c2 boundary and is one 16-byte load per
// source row; otherwise every column is loaded on its own, behind a safe address where it is outside its source.
template <bool VEC>
__device__ __forceinline__ void interp_fetch(const InterpSrc &s, const unsigned (&src)[3], long long row, long long row_end,
                                             int col, float4 (&d)[3])
{
    const long long r = row < row_end ? row : 0;
    if constexpr (VEC) {
        // branch-free for the two 16-byte forms: a chunk outside its source reads the first chunk of points2 and is dropped later
        const bool in2 = col < s.c2, ins = !in2 && col < s.c2 + s.c1;
        const int j = col - s.c2;
        const float *q0 = s.points2 + (in2 ? static_cast<size_t>(src[0]) * s.c2 + col : 0);
        const float *q1 = s.points2 + (in2 ? static_cast<size_t>(src[1]) * s.c2 + col : 0);
        const float *q2 = s.points2 + (in2 ? static_cast<size_t>(src[2]) * s.c2 + col : 0);
        if (ins && s.skip_vec) q0 = s.skip + r * s.c1 + j;
        d[0] = *reinterpret_cast<const float4 *>(q0);
        d[1] = *reinterpret_cast<const float4 *>(q1);
        d[2] = *reinterpret_cast<const float4 *>(q2);
        if (ins && !s.skip_vec) {   // c1 % 4 != 0 or an unaligned skip: its columns one by one
            const float *q = s.skip + r * s.c1;
            const bool k1 = j + 1 < s.c1, k2 = j + 2 < s.c1, k3 = j + 3 < s.c1;
            const float x = q[j], y = q[k1 ? j + 1 : 0], z = q[k2 ? j + 2 : 0], w = q[k3 ? j + 3 : 0];
            d[0] = make_float4(x, k1 ? y : 0.f, k2 ? z : 0.f, k3 ? w : 0.f);
        }
    } else {
        float x[3][4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int cj = col + i;
            const bool in2 = cj < s.c2, ins = !in2 && cj < s.c2 + s.c1;
            const float *q0 = in2 ? s.points2 + static_cast<size_t>(src[0]) * s.c2 + cj : (ins ? s.skip + r * s.c1 + (cj - s.c2) : s.points2);
            const float *q1 = in2 ? s.points2 + static_cast<size_t>(src[1]) * s.c2 + cj : s.points2;
            const float *q2 = in2 ? s.points2 + static_cast<size_t>(src[2]) * s.c2 + cj : s.points2;
            x[0][i] = *q0; x[1][i] = *q1; x[2][i] = *q2;
        }
#pragma unroll
        for (int t = 0; t < 3; ++t) d[t] = make_float4(x[t][0], x[t][1], x[t][2], x[t][3]);
    }
}

__device__ __forceinline__ float interp3(const float (&w)[3], float a, float b, float c)
{
    return w[0] * a + w[1] * b + w[2] * c;   // left to right, no contraction: as three_interpolate_concat_kernel
}

// the four operand values from what interp_fetch loaded; rows and columns outside the matrix are zero
template <bool VEC>
__device__ __forceinline__ float4 interp_combine(const InterpSrc &s, const float (&w)[3], bool row_ok, int col, const float4 (&d)[3])
{
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (!row_ok) return v;
    if constexpr (VEC) {
        if (col < s.c2) {
            v.x = interp3(w, d[0].x, d[1].x, d[2].x);
            v.y = interp3(w, d[0].y, d[1].y, d[2].y);
            v.z = interp3(w, d[0].z, d[1].z, d[2].z);
            v.w = interp3(w, d[0].w, d[1].w, d[2].w);
        } else if (col < s.c2 + s.c1) {
            v = d[0];
        }
    } else {
        const float a[4] = { d[0].x, d[0].y, d[0].z, d[0].w }, b[4] = { d[1].x, d[1].y, d[1].z, d[1].w },
                    c[4] = { d[2].x, d[2].y, d[2].z, d[2].w };
        float o[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int cj = col + i;
            o[i] = cj < s.c2 ? interp3(w, a[i], b[i], c[i]) : (cj < s.c2 + s.c1 ? a[i] : 0.f);
        }
        v = make_float4(o[0], o[1], o[2], o[3]);
    }
    return v;
}

// ------------------------------------------------------------------------------------------
// forward: Z = operand W^T + bias, partial BN statistics of Z per workgroup (linear_fwd_kernel of gemm.hip with the A loader
// above).  A thread stages the same four rows in every K stage of a tile: their indices and weights are loaded once per tile.
// ------------------------------------------------------------------------------------------
template <int NT, bool VEC>
__global__ __launch_bounds__(kGemmThreads) __attribute__((amdgpu_waves_per_eu(2))) void interp_linear_fwd_kernel(
    long long rows, int cin, int cout, long long ntiles, InterpSrc src, const float *__restrict__ W,
    const float *__restrict__ bias, float *__restrict__ Z, float *__restrict__ partial)
{
    __shared__ FwdLds<NT> lds;
    const int lane = threadIdx.x & 63;
    const int k4 = fwd_k4(), srow = fwd_srow();
    float s[NT][2] = {};

    unsigned ridx[4][3];    // source rows of the tile that the NEXT fetch reads
    float rw[4][3];         // weights of the tile whose loads are combined next
    float4 ar[4][3], br[NT];
    auto load_idx = [&](long long r0) {
#pragma unroll
        for (int p = 0; p < 4; ++p) interp_row_idx(src, r0 + srow + 32 * p, rows, ridx[p]);
    };
    auto load_w = [&](long long r0) {
#pragma unroll
        for (int p = 0; p < 4; ++p) interp_row_w(src, r0 + srow + 32 * p, rows, rw[p]);
    };
    // one stage's loads; when the fetch after this one belongs to the workgroup's next tile, that tile's indices are loaded
    // now (this tile's are not needed again), so that fetch finds them in registers
    auto fetch = [&](long long tile, int kc) {
        const long long r0 = tile * kFwdRows;
#pragma unroll
        for (int p = 0; p < 4; ++p) interp_fetch<VEC>(src, ridx[p], r0 + srow + 32 * p, rows, kc + k4, ar[p]);
#pragma unroll
        for (int p = 0; p < NT; ++p) br[p] = load4_guarded<VEC>(W, srow + 32 * p, cout, kc + k4, cin);
        if (kc + kFwdKC >= cin && tile + gridDim.x < ntiles) load_idx((tile + gridDim.x) * kFwdRows);
    };
    if (blockIdx.x < ntiles) {
        load_idx(static_cast<long long>(blockIdx.x) * kFwdRows);
        load_w(static_cast<long long>(blockIdx.x) * kFwdRows);
        fetch(blockIdx.x, 0);
    }
    for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const long long row0 = tile * kFwdRows;
        f32x16 acc[NT];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int g = 0; g < 16; ++g) acc[nt][g] = 0.f;

        for (int kc = 0; kc < cin; kc += kFwdKC) {
            // the multiplies happen here, not at fetch time: the gathered loads stay in flight across the MFMA loop
#pragma unroll
            for (int p = 0; p < 4; ++p)
                *reinterpret_cast<float4 *>(&lds.As[(srow + 32 * p) * kFwdLS + k4]) =
                    interp_combine<VEC>(src, rw[p], row0 + srow + 32 * p < rows, kc + k4, ar[p]);
#pragma unroll
            for (int p = 0; p < NT; ++p) *reinterpret_cast<float4 *>(&lds.Bs[(srow + 32 * p) * kFwdLS + k4]) = br[p];
            __syncthreads();
            // the next stage -- of this tile, or the first one of the workgroup's next tile -- is in flight during
            // the MFMAs and the output stores below
            if (kc + kFwdKC < cin) {
                fetch(tile, kc + kFwdKC);
            } else if (tile + gridDim.x < ntiles) {
                load_w((tile + gridDim.x) * kFwdRows);
                fetch(tile + gridDim.x, 0);
            }
            fwd_mfma_stage(lds, acc);
            __syncthreads();
        }
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const int col = nt * 32 + (lane & 31);
            const bool col_ok = col < cout;
            const float bv = (bias && col_ok) ? bias[col] : 0.f;
#pragma unroll
            for (int g = 0; g < 16; ++g) {
                const long long row = fwd_d_row(row0, g);
                const float v = acc[nt][g] + bv;
                if (col_ok && row < rows) {
                    Z[row * cout + col] = v;
                    s[nt][0] += v;
                    s[nt][1] += v * v;
                }
            }
        }
    }
    col_sums_store(lds, s, cout, partial);
}

// ------------------------------------------------------------------------------------------
// wgrad: partial[chunk][n][k] = sum over the chunk's rows of G[r][n] * operand[r][k] (wgrad_kernel of gemm.hip with the
// operand rebuilt).  Rows are the reduction here, so every stage brings new rows: the indices and weights of the stage after
// the one being fetched are loaded one stage ahead, and the gathered loads never wait for their addresses.
// ------------------------------------------------------------------------------------------
template <int WM, int WN, bool VEC>
__global__ __launch_bounds__(kGemmThreads) void interp_wgrad_kernel(long long rows, int cout, int cin, int mtiles,
                                                                    long long rows_per_chunk, const float *__restrict__ G,
                                                                    InterpSrc src, float *__restrict__ partial)
{
    using Q = WgradTile<WM, WN>;
    __shared__ typename Q::Lds lds;
    const Q q(rows, mtiles, rows_per_chunk);

    unsigned nidx[Q::XPASS][3];                 // source rows and weights of the stage that the next fetch reads
    float nw[Q::XPASS][3], cw[Q::XPASS][3];     // cw: weights of the stage whose loads are in xr
    float4 gr[Q::GPASS], xr[Q::XPASS][3];
    auto load_meta = [&](long long rt) {
#pragma unroll
        for (int p = 0; p < Q::XPASS; ++p) {
            interp_row_idx(src, rt + q.xrow + p * Q::XROWS, q.r1, nidx[p]);
            interp_row_w(src, rt + q.xrow + p * Q::XROWS, q.r1, nw[p]);
        }
    };
    auto fetch = [&](long long rt) {
#pragma unroll
        for (int p = 0; p < Q::GPASS; ++p) gr[p] = load4_guarded<VEC>(G, rt + q.grow + p * Q::GROWS, q.r1, q.gcol, cout);
#pragma unroll
        for (int p = 0; p < Q::XPASS; ++p) {
            interp_fetch<VEC>(src, nidx[p], rt + q.xrow + p * Q::XROWS, q.r1, q.xcol, xr[p]);
            cw[p][0] = nw[p][0]; cw[p][1] = nw[p][1]; cw[p][2] = nw[p][2];
        }
        load_meta(rt + kGemmRowsPerStage);
    };
    // the multiplies happen when the stage is stored, not at fetch time: the gathered loads stay in flight across the MFMA loop
    auto stage_x = [&](int p, long long rt) { return interp_combine<VEC>(src, cw[p], rt + q.xrow + p * Q::XROWS < q.r1, q.xcol, xr[p]); };
    load_meta(q.r0);
    wgrad_tile_loop<WM, WN>(lds, q, cout, cin, partial, gr, fetch, stage_x);
}

}  // namespace hf

using namespace hf;

// the A operand of an interpolating launch; HF_EINVAL when the arguments do not describe one
static int make_interp(long long rows, int c2, int c1, const float *points2, int m, long long rows_per_cloud, const int *idx,
                       const float *weight3, const float *skip, InterpSrc *s)
{
    if (rows <= 0 || rows >= (1ll << 32) || rows_per_cloud <= 0 || rows % rows_per_cloud != 0 || m < 1 || c2 < 1 || c2 > 1024 ||
        c1 < 0 || c1 > 1024 || !points2 || !idx || !weight3 || (c1 > 0 && !skip))
        return HF_EINVAL;
    if (rows / rows_per_cloud * m >= (1ll << 31)) return HF_EINVAL;   // rows of points2 are addressed with 32 bits
    s->points2 = points2; s->idx = idx; s->w3 = weight3; s->skip = skip;
    s->c2 = c2; s->c1 = c1; s->m = m;
    s->rows_per_cloud = static_cast<unsigned>(rows_per_cloud);
    s->skip_vec = c2 % 4 == 0 && c1 > 0 && vec4_ok(skip, c1);
    return HF_OK;
}

HF_API int hf_linear_bn_fwd_interp(long long rows, int c2, int c1, int cout, const float *points2, int m, long long rows_per_cloud,
                                   const int *idx, const float *weight3, const float *skip, const float *weight, const float *bias,
                                   float *z, float eps, float momentum, float *running_mean, float *running_var, float *mean,
                                   float *invstd, void *workspace, size_t workspace_bytes, hf_stream_t stream)
{
    InterpSrc src;
    if (const int rc = make_interp(rows, c2, c1, points2, m, rows_per_cloud, idx, weight3, skip, &src); rc != HF_OK) return rc;
    if (cout < 1 || cout > 256 || !weight || !z || !mean || !invstd) return HF_EINVAL;
    if (!workspace || workspace_bytes < hf_linear_bn_fwd_workspace(cout)) return HF_EINVAL;
    const int cin = (c2 + c1 + 3) & ~3;
    hipStream_t st = as_stream(stream);
    float *partial = static_cast<float *>(workspace);
    const long long ntiles = (rows + kFwdRows - 1) / kFwdRows;
    const bool vec = vec4_ok(points2, c2) && vec4_ok(weight, cin);
    const int nt = div_up(cout, 32);
    const int nblk = resident_grid(nt, ntiles);
#define HF_FWD(N, V)                                                                                                    \
    hipLaunchKernelGGL((interp_linear_fwd_kernel<N, V>), dim3(nblk), dim3(kGemmThreads), 0, st, rows, cin, cout, ntiles, src, \
                       weight, bias, z, partial)
#define HF_FWD_V(N)                                                                                                     \
    case N:                                                                                                             \
        if (vec) HF_FWD(N, true); else HF_FWD(N, false);                                                                \
        break
    switch (nt) {
        HF_FWD_V(1); HF_FWD_V(2); HF_FWD_V(3); HF_FWD_V(4); HF_FWD_V(5); HF_FWD_V(6); HF_FWD_V(7); HF_FWD_V(8);
        default: return HF_EINVAL;
    }
#undef HF_FWD_V
#undef HF_FWD
    launch_bn_stats_finalize(rows, cout, nblk, partial, eps, momentum, running_mean, running_var, mean, invstd, st);
    return launch_status();
}

HF_API int hf_linear_wgrad_interp(long long rows, int cout, int c2, int c1, const float *grad_z, const float *points2, int m,
                                  long long rows_per_cloud, const int *idx, const float *weight3, const float *skip,
                                  float *grad_weight, void *workspace, size_t workspace_bytes, hf_stream_t stream)
{
    InterpSrc src;
    if (const int rc = make_interp(rows, c2, c1, points2, m, rows_per_cloud, idx, weight3, skip, &src); rc != HF_OK) return rc;
    if (cout < 1 || cout > 256 || !grad_z || !grad_weight) return HF_EINVAL;
    const int cin = (c2 + c1 + 3) & ~3;
    if (!workspace || workspace_bytes < hf_linear_wgrad_workspace(rows, cout, cin)) return HF_EINVAL;
    const WgradPlan p = wgrad_plan(rows, cout, cin);
    if (p.chunks > 65535) return HF_EINVAL;
    hipStream_t st = as_stream(stream);
    float *partial = static_cast<float *>(workspace);
    const dim3 grid(p.mtiles * p.ntiles, p.chunks);
    const bool vec = vec4_ok(grad_z, cout) && vec4_ok(points2, c2);
#define HF_WGRAD(M, N, V)                                                                                               \
    hipLaunchKernelGGL((interp_wgrad_kernel<M, N, V>), grid, dim3(kGemmThreads), 0, st, rows, cout, cin, p.mtiles,       \
                       p.rows_per_chunk, grad_z, src, partial)
#define HF_WGRAD_V(M, N)                                                                                                \
    do {                                                                                                                \
        if (vec) HF_WGRAD(M, N, true); else HF_WGRAD(M, N, false);                                                      \
    } while (0)
    if (p.wm == 2 && p.wn == 2) HF_WGRAD_V(2, 2);
    else if (p.wm == 2) HF_WGRAD_V(2, 1);
    else if (p.wn == 2) HF_WGRAD_V(1, 2);
    else HF_WGRAD_V(1, 1);
#undef HF_WGRAD_V
#undef HF_WGRAD
    launch_partial_reduce(cout * cin, p.chunks, partial, grad_weight, st);
    return launch_status();
}
