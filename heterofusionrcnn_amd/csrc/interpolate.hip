// interpolate.hip -- three_nn / three_interpolate (+grad) for gfx950.
//
// Replaces interpolate/tf_interpolate_g.cu:22-65,90-110,133-155 of the reference.
//
// three_nn: the reference keeps its three best distances in `double` initialised to 1e40
// (tf_interpolate_g.cu:43).  Once assigned they hold exact floats, and `d < 1e40` is true for
// every finite float d and false for +inf, which is exactly `d < +inf` in fp32; the float
// result of (float)1e40 is +inf.  So fp32 accumulators with a +inf sentinel are bit-equivalent.
#include <math.h>

#include <algorithm>

#include "hf_common.h"
#include "row_gather.h"

namespace hf {

constexpr int kNnThreads = 256;
constexpr int kNnTile = 2048;  // known points per LDS tile (24 KB)

__global__ __launch_bounds__(kNnThreads) void three_nn_kernel(int n, int m, const float *__restrict__ unknown,
                                                              const float *__restrict__ known,
                                                              float *__restrict__ dist2, int *__restrict__ idx)
{
    __shared__ float tile[kNnTile * 3];
    const int t = threadIdx.x;
    const int bb = blockIdx.y;
    const int j = blockIdx.x * kNnThreads + t;
    const float *u = unknown + static_cast<size_t>(bb) * n * 3;
    const float *kn = known + static_cast<size_t>(bb) * m * 3;
    const bool live = j < n;
    float ux = 0.f, uy = 0.f, uz = 0.f;
    if (live) { ux = u[j * 3 + 0]; uy = u[j * 3 + 1]; uz = u[j * 3 + 2]; }
    float b1 = INFINITY, b2 = INFINITY, b3 = INFINITY;
    int i1 = 0, i2 = 0, i3 = 0;
    for (int base = 0; base < m; base += kNnTile) {
        const int tn = min(kNnTile, m - base);
        __syncthreads();
        for (int e = t; e < tn * 3; e += kNnThreads) tile[e] = kn[static_cast<size_t>(base) * 3 + e];
        __syncthreads();
        for (int k = 0; k < tn; ++k) {
            const float x = tile[k * 3 + 0], y = tile[k * 3 + 1], z = tile[k * 3 + 2];
            const float dx = ux - x, dy = uy - y, dz = uz - z;
            const float d = dx * dx + dy * dy + dz * dz;
            if (d < b3) {  // rare after warm-up: the common path is one compare
                const int kk = base + k;
                if (d < b1) {
                    b3 = b2; i3 = i2;
                    b2 = b1; i2 = i1;
                    b1 = d; i1 = kk;
                } else if (d < b2) {
                    b3 = b2; i3 = i2;
                    b2 = d; i2 = kk;
                } else {
                    b3 = d; i3 = kk;
                }
            }
        }
    }
    if (live) {
        float *od = dist2 + (static_cast<size_t>(bb) * n + j) * 3;
        int *oi = idx + (static_cast<size_t>(bb) * n + j) * 3;
        od[0] = b1; od[1] = b2; od[2] = b3;
        oi[0] = i1; oi[1] = i2; oi[2] = i3;
    }
}

// channel-first op layout: points (b,c,m) -> out (b,c,n)   (tf_interpolate_g.cu:90-110)
__global__ void three_interpolate_cf_kernel(int c, int m, int n, const float *__restrict__ points,
                                            const int *__restrict__ idx, const float *__restrict__ weight,
                                            float *__restrict__ out)
{
    const int bb = blockIdx.z, cc = blockIdx.y;
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const float *w = weight + (static_cast<size_t>(bb) * n + j) * 3;
    const int *k = idx + (static_cast<size_t>(bb) * n + j) * 3;
    const float *p = points + (static_cast<size_t>(bb) * c + cc) * m;
    out[(static_cast<size_t>(bb) * c + cc) * n + j] = w[0] * p[k[0]] + w[1] * p[k[1]] + w[2] * p[k[2]];
}

__global__ void three_interpolate_cf_grad_kernel(int c, int n, int m, const float *__restrict__ grad_out,
                                                 const int *__restrict__ idx, const float *__restrict__ weight,
                                                 float *__restrict__ grad_points)
{
    const int bb = blockIdx.z, cc = blockIdx.y;
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const float *w = weight + (static_cast<size_t>(bb) * n + j) * 3;
    const int *k = idx + (static_cast<size_t>(bb) * n + j) * 3;
    float *g = grad_points + (static_cast<size_t>(bb) * c + cc) * m;
    const float go = grad_out[(static_cast<size_t>(bb) * c + cc) * n + j];
    atomicAdd(g + k[0], go * w[0]);
    atomicAdd(g + k[1], go * w[1]);
    atomicAdd(g + k[2], go * w[2]);
}

// channel-last (the Python surface's layout): points (b,m,c) -> out (b,n,c) and its two gradients are the weighted (NSRC = 3)
// instances of the row-gather family: row_gather.h

// three_interpolate written straight into the concat of pointnet_fp_module (pointnet_util.py:311-313):
//   out[b,j,:] = [ sum_t w_t * points[b, idx_t, 0:c], skip[b,j,0:c1], 0 ... ]      (row width `width`, multiple of 4)
// One float4 of output per lane; VEC4: c % 4 == 0, so a float4 never straddles the two sources.
template <bool VEC4>
__global__ void three_interpolate_concat_kernel(int m, int c, int c1, int w4, long long n_per_batch, long long nrows,
                                                const float *__restrict__ points, const int *__restrict__ idx,
                                                const float *__restrict__ weight, const float *__restrict__ skip,
                                                float *__restrict__ out)
{
    const long long total = nrows * w4;
    for (long long e = blockIdx.x * static_cast<long long>(blockDim.x) + threadIdx.x; e < total;
         e += static_cast<long long>(gridDim.x) * blockDim.x) {
        const long long row = e / w4;
        const int q = static_cast<int>(e - row * w4);
        const long long bb = row / n_per_batch;
        const int *k = idx + row * 3;
        const float *w = weight + row * 3;
        const float *base = points + bb * m * c;
        float v[4];
        if (VEC4 && q * 4 + 3 < c) {
            const float4 p0 = *reinterpret_cast<const float4 *>(base + static_cast<size_t>(k[0]) * c + q * 4);
            const float4 p1 = *reinterpret_cast<const float4 *>(base + static_cast<size_t>(k[1]) * c + q * 4);
            const float4 p2 = *reinterpret_cast<const float4 *>(base + static_cast<size_t>(k[2]) * c + q * 4);
            v[0] = w[0] * p0.x + w[1] * p1.x + w[2] * p2.x;  // left to right, no contraction: as three_interpolate
            v[1] = w[0] * p0.y + w[1] * p1.y + w[2] * p2.y;
            v[2] = w[0] * p0.z + w[1] * p1.z + w[2] * p2.z;
            v[3] = w[0] * p0.w + w[1] * p1.w + w[2] * p2.w;
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int j = q * 4 + i;
                if (j < c)
                    v[i] = w[0] * base[static_cast<size_t>(k[0]) * c + j] + w[1] * base[static_cast<size_t>(k[1]) * c + j] +
                           w[2] * base[static_cast<size_t>(k[2]) * c + j];
                else if (j < c + c1)
                    v[i] = skip[row * c1 + (j - c)];
                else
                    v[i] = 0.0f;
            }
        }
        *reinterpret_cast<float4 *>(out + e * 4) = make_float4(v[0], v[1], v[2], v[3]);
    }
}

// ------------------------------------------------------------------------------------------
// Inverse of a three_nn index (CSR over the known points) and the gather form of the interpolation gradient.
// The scatter form (row_gather.h) issues 3*N*C float atomics; with the inverse each known point sums its referencing
// rows in registers and writes once, in ascending (unknown point, slot) order -- the accumulation order of the
// sequential loop in tf_interpolate.cpp:150-167, so the result is deterministic and matches it bit for bit.
// One 1024-thread workgroup per cloud: counts and cursors live in LDS (2*m ints).
// ------------------------------------------------------------------------------------------
constexpr int kInvThreads = 1024;
constexpr int kInvMaxKnown = 8192;        // three_nn_inverse (ABI limit kept); the general form takes up to kInvMaxTargets
constexpr int kInvMaxTargets = 19968;     // 2 ints of LDS per target: 156 KB

// `total` index values per cloud, each in [0, m): the CSR inverse (for every target the flat positions that name it, ascending).
// three_nn: total = 3 n; group_point / kNN tables: total = queries * nsample.
__global__ __launch_bounds__(kInvThreads) void three_nn_inverse_kernel(long long total, int m, const int *__restrict__ idx,
                                                                       int *__restrict__ offsets,
                                                                       int *__restrict__ entries)
{
    extern __shared__ int inv_lds[];
    __shared__ int wsum[16];
    int *cnt = inv_lds, *cur = inv_lds + m;
    const int b = blockIdx.x, t = threadIdx.x;
    const int *ib = idx + b * total;
    int *off = offsets + static_cast<long long>(b) * (m + 1);
    int *ent = entries + b * total;
    for (int i = t; i < m; i += kInvThreads) cnt[i] = 0;
    __syncthreads();
    for (long long e = t; e < total; e += kInvThreads) {
        const int k = ib[e];
        if (k >= 0 && k < m) atomicAdd(&cnt[k], 1);
    }
    __syncthreads();
    int carry = 0;
    for (int base = 0; base < m; base += kInvThreads) {
        const int i = base + t;
        const int v = i < m ? cnt[i] : 0;
        int tot;
        const int ex = block_exclusive_scan(v, wsum, &tot);
        if (i < m) {
            cur[i] = carry + ex;
            off[i] = carry + ex;
        }
        carry += tot;
    }
    if (t == 0) off[m] = carry;
    __syncthreads();
    for (long long e = t; e < total; e += kInvThreads) {
        const int k = ib[e];
        if (k >= 0 && k < m) ent[atomicAdd(&cur[k], 1)] = static_cast<int>(e);
    }
    __syncthreads();  // bucket contents (global memory) visible to the whole workgroup
    // ascending order inside every bucket: insertion sort, buckets hold ~3n/m entries
    for (int i = t; i < m; i += kInvThreads) {
        const int lo = cur[i] - cnt[i], hi = cur[i];
        for (int a = lo + 1; a < hi; ++a) {
            const int v = ent[a];
            int p = a - 1;
            while (p >= lo && ent[p] > v) {
                ent[p + 1] = ent[p];
                --p;
            }
            ent[p + 1] = v;
        }
    }
}

}  // namespace hf

using namespace hf;

HF_API int hf_three_nn(int b, int n, int m, const float *unknown, const float *known, float *dist2, int *idx,
                       hf_stream_t stream)
{
    // ThreeNNGpuOp: (b,n,3) / (b,m,3)  (tf_interpolate.cpp:68-75)
    if (b < 0 || n < 0 || m <= 0 || !unknown || !known || !dist2 || !idx) return HF_EINVAL;
    if (b == 0 || n == 0) return HF_OK;
    if (b > 65535) return HF_EINVAL;
    hipLaunchKernelGGL(three_nn_kernel, dim3(div_up(n, kNnThreads), b), dim3(kNnThreads), 0, as_stream(stream), n, m,
                       unknown, known, dist2, idx);
    return launch_status();
}

HF_API int hf_three_interpolate(int b, int c, int m, int n, const float *points, const int *idx, const float *weight,
                                float *out, hf_stream_t stream)
{
    if (b < 0 || c <= 0 || m <= 0 || n < 0 || !points || !idx || !weight || !out) return HF_EINVAL;
    if (b == 0 || n == 0) return HF_OK;
    if (b > 65535 || c > 65535) return HF_EINVAL;
    hipLaunchKernelGGL(three_interpolate_cf_kernel, dim3(div_up(n, 256), c, b), dim3(256), 0, as_stream(stream), c, m,
                       n, points, idx, weight, out);
    return launch_status();
}

HF_API int hf_three_interpolate_grad(int b, int c, int n, int m, const float *grad_out, const int *idx,
                                     const float *weight, float *grad_points, hf_stream_t stream)
{
    if (b < 0 || c <= 0 || m <= 0 || n < 0 || !grad_out || !idx || !weight || !grad_points) return HF_EINVAL;
    if (b == 0) return HF_OK;
    if (b > 65535 || c > 65535) return HF_EINVAL;
    hipStream_t st = as_stream(stream);
    int rc = hip_status(hipMemsetAsync(grad_points, 0, sizeof(float) * static_cast<size_t>(b) * c * m, st));
    if (rc != HF_OK) return rc;
    if (n == 0) return HF_OK;
    hipLaunchKernelGGL(three_interpolate_cf_grad_kernel, dim3(div_up(n, 256), c, b), dim3(256), 0, st, c, n, m,
                       grad_out, idx, weight, grad_points);
    return launch_status();
}

HF_API int hf_three_interpolate_cl(int b, int m, int c, int n, const float *points, const int *idx,
                                   const float *weight, float *out, hf_stream_t stream)
{
    if (b < 0 || c <= 0 || m <= 0 || n < 0 || !points || !idx || !weight || !out) return HF_EINVAL;
    if (static_cast<long long>(b) * n == 0) return HF_OK;
    return launch_gather_rows<3>(true, b, m, c, n, c, 0, points, idx, weight, out, as_stream(stream));
}

HF_API int hf_three_interpolate_cl_grad(int b, int n, int c, int m, const float *grad_out, const int *idx,
                                        const float *weight, float *grad_points, hf_stream_t stream)
{
    if (b < 0 || c <= 0 || m <= 0 || n < 0 || !grad_out || !idx || !weight || !grad_points) return HF_EINVAL;
    if (b == 0) return HF_OK;
    hipStream_t st = as_stream(stream);
    const int rc = hip_status(hipMemsetAsync(grad_points, 0, sizeof(float) * static_cast<size_t>(b) * m * c, st));
    if (rc != HF_OK || n == 0) return rc;
    return launch_scatter_rows<3>(b, m, c, n, c, 0, grad_out, idx, weight, grad_points, st);
}

// `total` index values per cloud, each in [0, m): one launch for both inverse entry points, which keep their own limits on m
static int launch_index_inverse(int b, long long total, int m, const int *idx, int *offsets, int *entries, hipStream_t st)
{
    const size_t lds = sizeof(int) * 2 * static_cast<size_t>(m);   // m = 8192: 64 KB, above the default limit
    const int lrc = ensure_dynamic_lds(reinterpret_cast<const void *>(&three_nn_inverse_kernel), lds);
    if (lrc != HF_OK) return lrc;
    hipLaunchKernelGGL(three_nn_inverse_kernel, dim3(b), dim3(kInvThreads), lds, st, total, m, idx, offsets, entries);
    return launch_status();
}

HF_API int hf_three_nn_inverse(int b, int n, int m, const int *idx, int *offsets, int *entries, hf_stream_t stream)
{
    if (b < 0 || n < 0 || m <= 0 || m > kInvMaxKnown || !offsets || (n > 0 && (!idx || !entries))) return HF_EINVAL;
    if (b == 0) return HF_OK;
    if (static_cast<long long>(n) * 3 > 0x7fffffffll) return HF_EINVAL;
    return launch_index_inverse(b, 3ll * n, m, idx, offsets, entries, as_stream(stream));
}

HF_API int hf_index_inverse(int b, long long total, int m, const int *idx, int *offsets, int *entries, hf_stream_t stream)
{
    if (b < 0 || total < 0 || m <= 0 || m > kInvMaxTargets || total > 0x7fffffffll || !offsets || (total > 0 && (!idx || !entries)))
        return HF_EINVAL;
    if (b == 0) return HF_OK;
    return launch_index_inverse(b, total, m, idx, offsets, entries, as_stream(stream));
}

// both gather-form gradient entries: grad_out rows of stride ld >= c, the interpolated columns first
static int interpolate_grad_gather(int b, int n, int c, int ld, int m, const float *grad_out, const float *weight,
                                   const int *offsets, const int *entries, float *grad_points, hf_stream_t stream)
{
    if (b < 0 || n < 0 || c < 0 || ld < c || m <= 0 || !offsets || !grad_points ||
        (n > 0 && c > 0 && (!grad_out || !weight || !entries)))
        return HF_EINVAL;
    if (b == 0 || c == 0) return HF_OK;
    return launch_grad_gather_rows<3>(b, m, c, n, ld, 0, grad_out, weight, offsets, entries, grad_points, as_stream(stream));
}

HF_API size_t hf_three_nn_workspace(int b, int m)
{
    return knn_grid_workspace(b, m);  // 0: larger clouds use the all-pairs kernel
}

// three_nn IS the 3-nearest-neighbour search with the reference's conventions: squared distances ascending, ties to
// the lower index (strict `<` over ascending k, tf_interpolate_g.cu:43-62), +inf / index 0 in the slots that fewer
// than three known points leave empty -- exactly what the grid kNN kernel (grouping.hip) produces for k = 3.
HF_API int hf_three_nn_sorted(int b, int n, int m, const float *unknown, const float *known, float *dist2, int *idx,
                              void *workspace, size_t workspace_bytes, hf_stream_t stream)
{
    if (b < 0 || n < 0 || m <= 0 || !unknown || !known || !dist2 || !idx) return HF_EINVAL;
    if (b == 0 || n == 0) return HF_OK;
    if (b > 65535) return HF_EINVAL;
    const size_t need = hf_three_nn_workspace(b, m);
    if (need == 0) return hf_three_nn(b, n, m, unknown, known, dist2, idx, stream);
    if (!workspace || workspace_bytes < need) return HF_EWORKSPACE;
    return launch_knn_grid(b, m, n, 3, known, unknown, dist2, idx, workspace, as_stream(stream));
}

HF_API int hf_three_interpolate_cl_grad_gather(int b, int n, int c, int m, const float *grad_out, const float *weight,
                                               const int *offsets, const int *entries, float *grad_points,
                                               hf_stream_t stream)
{
    return interpolate_grad_gather(b, n, c, c, m, grad_out, weight, offsets, entries, grad_points, stream);
}

HF_API int hf_three_interpolate_concat(int b, int m, int c, int n, int c1, int width, const float *points, const int *idx,
                                       const float *weight, const float *skip, float *out, hf_stream_t stream)
{
    if (b < 0 || c <= 0 || m <= 0 || n < 0 || c1 < 0 || width < c + c1 || width % 4 != 0) return HF_EINVAL;
    const long long nrows = static_cast<long long>(b) * n;
    if (nrows == 0) return HF_OK;  // empty tensors carry null pointers
    if (!points || !idx || !weight || !out || (c1 > 0 && !skip) || reinterpret_cast<uintptr_t>(out) % 16 != 0) return HF_EINVAL;
    const int block = 256;
    const dim3 grid(grid_for(nrows * (width / 4), block));
    const bool vec4 = c % 4 == 0 && reinterpret_cast<uintptr_t>(points) % 16 == 0;
    if (vec4)
        hipLaunchKernelGGL((three_interpolate_concat_kernel<true>), grid, dim3(block), 0, as_stream(stream), m, c, c1, width / 4,
                           static_cast<long long>(n), nrows, points, idx, weight, skip, out);
    else
        hipLaunchKernelGGL((three_interpolate_concat_kernel<false>), grid, dim3(block), 0, as_stream(stream), m, c, c1,
                           width / 4, static_cast<long long>(n), nrows, points, idx, weight, skip, out);
    return launch_status();
}

HF_API int hf_three_interpolate_concat_grad(int b, int n, int c, int m, int width, const float *grad_out, const float *weight,
                                            const int *offsets, const int *entries, float *grad_points, hf_stream_t stream)
{
    return interpolate_grad_gather(b, n, c, width, m, grad_out, weight, offsets, entries, grad_points, stream);
}
