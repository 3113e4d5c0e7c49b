// row_gather.h -- the row-gather family shared by grouping.hip (group_point*), interpolate.hip (three_interpolate_cl*) and
// sampling.hip (gather_point*): four kernel templates and one host launcher for each.
//
// One idea: for every output row fetch NSRC source rows named by an index -- NSRC = 1: a copy; NSRC = 3: the weighted sum of
// three -- and write the result to columns [col, col + c) of a row of `width` floats.  Its gradient has two forms: scatter with
// atomics into a zero-filled target (the reference's form), and gather over the CSR inverse of the index (hf_index_inverse /
// hf_three_nn_inverse): every target row sums the rows that name it in registers and is written once.
//
// Rules of the family, stated here once:
//   * values     copy forms move bits (NaN payloads, signed zeros and denormals pass through; nothing is multiplied by one);
//                weighted forward  w0*p0 + w1*p1 + w2*p2  left to right; scatter  go * w_t  then atomicAdd; gather form
//                acc += v * w[e]  (copy: acc += v) in ascending entry order = the order of the reference's sequential loops,
//                which is what makes it bit-equal to them.  The library is built with -ffp-contract=off.
//   * alignment  16-byte accesses need c, width and col multiples of 4 and both the table and the strided operand 16-byte
//                aligned; anything else takes the one-float-per-lane form of the same kernel.
//   * pow2 form  only for dense output rows (width == c, col == 0) from the entries that ask for it, c / 4 a power of two in
//                4 .. 256, b <= 65535, rows_per_batch * c / 4 < 2^31; rows past the end of a cloud re-read the thread's first
//                row (`row < rows ? row : row0`) and are not stored.
//   * grids      grid_for (hf_common.h): at most 8 workgroups per CU, grid-stride loops cover the rest; the pow2 form shares
//                that cap between the clouds; the gather-form gradient takes up to 64 per CU.
//   * targets    the scatter form adds into a target that the entry point zero-fills; the gather form writes every target row
//                (one that nothing names becomes +0) and needs no fill.
#pragma once
#include <algorithm>

#include "hf_common.h"

namespace hf {

// VEC floats of a row; a plain float for VEC = 1
template <int VEC> struct RowVec { typedef float type __attribute__((ext_vector_type(VEC))); };
template <> struct RowVec<1> { typedef float type; };

// out[row][col + ...] = points[bb][idx[row * NSRC + t]][...] (weighted by weight[row * NSRC + t] for NSRC = 3); VEC floats per
// lane, c / VEC lanes per row, so that both the gathered segments and the destination are contiguous.  n: source rows per
// cloud.  CFIX != 0: c is that constant (gather_point's c = 3: no run-time division by the row length).
template <int NSRC, int VEC, int CFIX = 0>
__global__ void gather_rows_kernel(int n, int c_arg, int width, int col, long long rows_per_batch, long long nrows,
                                   const float *__restrict__ points, const int *__restrict__ idx,
                                   const float *__restrict__ weight, float *__restrict__ out)
{
    typedef typename RowVec<VEC>::type vec_t;
    const int c = CFIX ? CFIX : c_arg;
    const int cv = c / VEC;  // vectors per row
    const long long total = nrows * cv;
    for (long long e = blockIdx.x * static_cast<long long>(blockDim.x) + threadIdx.x; e < total;
         e += static_cast<long long>(gridDim.x) * blockDim.x) {
        const long long row = e / cv;
        const int l = static_cast<int>(e - row * cv) * VEC;
        const long long bb = row / rows_per_batch;
        const float *base = points + bb * n * c + l;
        const int *k = idx + row * NSRC;
        vec_t r;
        if constexpr (NSRC == 1) {
            r = *reinterpret_cast<const vec_t *>(base + static_cast<long long>(k[0]) * c);
        } else {
            const float *w = weight + row * NSRC;
            const vec_t p0 = *reinterpret_cast<const vec_t *>(base + static_cast<long long>(k[0]) * c);
            const vec_t p1 = *reinterpret_cast<const vec_t *>(base + static_cast<long long>(k[1]) * c);
            const vec_t p2 = *reinterpret_cast<const vec_t *>(base + static_cast<long long>(k[2]) * c);
            r = w[0] * p0 + w[1] * p1 + w[2] * p2;  // left to right, no contraction
        }
        *reinterpret_cast<vec_t *>(out + row * width + col + l) = r;
    }
}

// The same op on dense output rows when c / 4 is a power of two (c = 16 .. 1024, every width the reference configs use): no
// integer division (lane -> row by a shift), ROWS rows per thread in flight (the index and weight loads, then NSRC * ROWS
// independent 16-byte gathers before the first use), nontemporal stores for the write-once output so that the table (a few MB
// per cloud) stays in the XCD's L2.  Consecutive lanes cover consecutive 16-byte pieces of consecutive rows.
template <int NSRC, int ROWS>
__global__ __launch_bounds__(256) void gather_rows_pow2_kernel(int nbatch, int n, int c, int cv_shift, int rows_per_batch,
                                                               const float *__restrict__ points, const int *__restrict__ idx,
                                                               const float *__restrict__ weight, float *__restrict__ out)
{
    typedef float v4 __attribute__((ext_vector_type(4)));
    // linear workgroup id = cloud + b * chunk: workgroups are dealt round-robin over the 8 XCDs, so with b a multiple of 8
    // every workgroup of a cloud runs on ONE XCD and that cloud's table stays in its 4 MB L2 (speed only)
    const int bb = blockIdx.x % nbatch;
    const unsigned gxb = gridDim.x / nbatch;
    const unsigned tid = (blockIdx.x / nbatch) * 256u + threadIdx.x;
    const int l = static_cast<int>(tid & ((1u << cv_shift) - 1u));
    const int rstride = static_cast<int>((gxb * 256u) >> cv_shift);
    const float *base = points + static_cast<size_t>(bb) * n * c + l * 4;
    const int *kb = idx + static_cast<size_t>(bb) * rows_per_batch * NSRC;
    const float *wb = weight + static_cast<size_t>(bb) * rows_per_batch * NSRC;
    float *ob = out + static_cast<size_t>(bb) * rows_per_batch * c + l * 4;
    for (int row0 = static_cast<int>(tid >> cv_shift); row0 < rows_per_batch; row0 += rstride * ROWS) {
        v4 p[ROWS][NSRC];
        [[maybe_unused]] float w[ROWS][NSRC];
#pragma unroll
        for (int i = 0; i < ROWS; ++i) {
            const int row = row0 + i * rstride;
            const int rr = row < rows_per_batch ? row : row0;
#pragma unroll
            for (int t = 0; t < NSRC; ++t) {
                if constexpr (NSRC == 3) w[i][t] = wb[rr * NSRC + t];
                p[i][t] = *reinterpret_cast<const v4 *>(base + static_cast<size_t>(kb[rr * NSRC + t]) * c);
            }
        }
#pragma unroll
        for (int i = 0; i < ROWS; ++i) {
            const int row = row0 + i * rstride;
            if (row < rows_per_batch) {
                v4 r;
                if constexpr (NSRC == 1) r = p[i][0];
                else r = w[i][0] * p[i][0] + w[i][1] * p[i][1] + w[i][2] * p[i][2];  // left to right, no contraction
                __builtin_nontemporal_store(r, reinterpret_cast<v4 *>(ob + static_cast<size_t>(row) * c));
            }
        }
    }
}

// The gradient in scatter form (the reference's atomicAdd loops): grad_out[row][col + l] (times weight[row * 3 + t]) added to
// row idx[row * NSRC + t] of the target, which the caller has zero-filled.  One lane per float.  n: target rows per cloud.
template <int NSRC, int CFIX = 0>
__global__ void scatter_rows_kernel(int n, int c_arg, int width, int col, long long rows_per_batch, long long nrows,
                                    const float *__restrict__ grad_out, const int *__restrict__ idx,
                                    const float *__restrict__ weight, float *__restrict__ grad_points)
{
    const int c = CFIX ? CFIX : c_arg;
    const long long total = nrows * c;
    for (long long e = blockIdx.x * static_cast<long long>(blockDim.x) + threadIdx.x; e < total;
         e += static_cast<long long>(gridDim.x) * blockDim.x) {
        const long long row = e / c;
        const int l = static_cast<int>(e - row * c);
        const long long bb = row / rows_per_batch;
        const int *k = idx + row * NSRC;
        const float go = grad_out[row * width + col + l];
        float *g = grad_points + bb * n * c + l;
        if constexpr (NSRC == 1) {
            atomicAdd(g + static_cast<long long>(k[0]) * c, go);
        } else {
            const float *w = weight + row * NSRC;
            atomicAdd(g + static_cast<long long>(k[0]) * c, go * w[0]);
            atomicAdd(g + static_cast<long long>(k[1]) * c, go * w[1]);
            atomicAdd(g + static_cast<long long>(k[2]) * c, go * w[2]);
        }
    }
}

// The gradient in gather form: for every target row the entries that name it (CSR inverse of the index: offsets (b, n + 1),
// entries (b, rows_per_batch * NSRC), ascending inside a bucket) are summed in that order -- the order of the reference's
// sequential CPU loops (grouping/test/query_ball_point.cpp:53-66, tf_interpolate.cpp:150-167) -- and the row is written ONCE:
// no atomics, no zero fill, deterministic.  Entry e stands for row e / NSRC of grad_out (row stride ld, columns from col) and,
// for NSRC = 3, weight w[e].  cv = c / VEC lanes per target row.
template <int NSRC, int VEC>
__global__ void grad_gather_rows_kernel(int n, int c, int ld, int col, int cv, long long rows_per_batch, long long target_rows,
                                        const float *__restrict__ grad_out, const float *__restrict__ weight,
                                        const int *__restrict__ offsets, const int *__restrict__ entries,
                                        float *__restrict__ grad_points)
{
    const int rows_per_block = blockDim.x / cv;
    const int cvec = threadIdx.x % cv, rsub = threadIdx.x / cv;
    if (rsub >= rows_per_block) return;
    for (long long row = blockIdx.x * static_cast<long long>(rows_per_block) + rsub; row < target_rows;
         row += static_cast<long long>(gridDim.x) * rows_per_block) {
        const long long bb = row / n;
        const int k = static_cast<int>(row - bb * n);
        const int *off = offsets + bb * (n + 1);
        const int *ent = entries + bb * rows_per_batch * NSRC;
        const float *go = grad_out + bb * rows_per_batch * ld + col + cvec * VEC;
        const float *w = weight + bb * rows_per_batch * NSRC;
        float acc[VEC];
#pragma unroll
        for (int i = 0; i < VEC; ++i) acc[i] = 0.0f;
        const int lo = off[k], hi = off[k + 1];
        for (int a = lo; a < hi; ++a) {
            const int e = ent[a];
            const float *src = go + static_cast<long long>(e / NSRC) * ld;
            if constexpr (NSRC == 1) {
                if constexpr (VEC == 4) {
                    const float4 v = *reinterpret_cast<const float4 *>(src);
                    acc[0] += v.x; acc[1] += v.y; acc[2] += v.z; acc[3] += v.w;
                } else {
                    acc[0] += src[0];
                }
            } else {
                const float wt = w[e];
                if constexpr (VEC == 4) {
                    const float4 v = *reinterpret_cast<const float4 *>(src);
                    acc[0] += v.x * wt; acc[1] += v.y * wt; acc[2] += v.z * wt; acc[3] += v.w * wt;
                } else {
                    acc[0] += src[0] * wt;
                }
            }
        }
        float *dst = grad_points + row * c + cvec * VEC;
        if constexpr (VEC == 4) *reinterpret_cast<float4 *>(dst) = make_float4(acc[0], acc[1], acc[2], acc[3]);
        else dst[0] = acc[0];
    }
}

// ---- host launchers: shapes are checked by the entry points; b, rows_per_batch > 0 ----

inline bool aligned16(const void *a, const void *b) { return (reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) % 16 == 0; }

// The regime choice of the forward gather, written once: pow2 (only where the entry point allows it), 16-byte, scalar.
template <int NSRC, int CFIX = 0>
inline int launch_gather_rows(bool allow_pow2, int b, int n, int c, long long rows_per_batch, int width, int col, const float *points,
                              const int *idx, const float *weight, float *out, hipStream_t st)
{
    const long long nrows = b * rows_per_batch;
    const int block = 256, cv = c / 4;
    const bool vec4 = c % 4 == 0 && width % 4 == 0 && col % 4 == 0 && aligned16(points, out);
    if (allow_pow2 && vec4 && width == c && col == 0 && cv >= 4 && cv <= 256 && (cv & (cv - 1)) == 0 && b <= 65535 &&
        rows_per_batch * cv < (1LL << 31)) {
        int cv_shift = 0;
        while ((1 << cv_shift) < cv) ++cv_shift;
        // 4 rows in flight per thread; enough workgroups for ~8 per CU across the batch
        long long gx = (rows_per_batch * cv + 256 * 4 - 1) / (256 * 4);
        const long long cap = std::max<long long>(1, (kNumCU * 8) / b);
        if (gx > cap) gx = cap;
        hipLaunchKernelGGL((gather_rows_pow2_kernel<NSRC, 4>), dim3(static_cast<unsigned>(gx * b)), dim3(256), 0, st, b, n, c, cv_shift,
                           static_cast<int>(rows_per_batch), points, idx, weight, out);
    } else if (vec4)
        hipLaunchKernelGGL((gather_rows_kernel<NSRC, 4>), dim3(grid_for(nrows * cv, block)), dim3(block), 0, st, n, c, width, col,
                           rows_per_batch, nrows, points, idx, weight, out);
    else
        hipLaunchKernelGGL((gather_rows_kernel<NSRC, 1, CFIX>), dim3(grid_for(nrows * c, block)), dim3(block), 0, st, n, c, width, col,
                           rows_per_batch, nrows, points, idx, weight, out);
    return launch_status();
}

template <int NSRC, int CFIX = 0>
inline int launch_scatter_rows(int b, int n, int c, long long rows_per_batch, int width, int col, const float *grad_out, const int *idx,
                               const float *weight, float *grad_points, hipStream_t st)
{
    const long long nrows = b * rows_per_batch;
    const int block = 256;
    hipLaunchKernelGGL((scatter_rows_kernel<NSRC, CFIX>), dim3(grid_for(nrows * c, block)), dim3(block), 0, st, n, c, width, col,
                       rows_per_batch, nrows, grad_out, idx, weight, grad_points);
    return launch_status();
}

// HF_EINVAL: a row longer than 1024 lanes (c > 4096, or > 1024 where 16-byte accesses are not possible)
template <int NSRC>
inline int launch_grad_gather_rows(int b, int n, int c, long long rows_per_batch, int ld, int col, const float *grad_out,
                                   const float *weight, const int *offsets, const int *entries, float *grad_points, hipStream_t st)
{
    const long long target_rows = static_cast<long long>(b) * n;
    const bool vec4 = c % 4 == 0 && ld % 4 == 0 && col % 4 == 0 && aligned16(grad_out, grad_points);
    const int cv = vec4 ? c / 4 : c;
    if (cv > 1024) return HF_EINVAL;
    int block = 256;
    if (cv > block) block = ((cv + 63) / 64) * 64;
    const int rows_per_block = block / cv;
    long long grid = (target_rows + rows_per_block - 1) / rows_per_block;
    if (grid > kNumCU * 64ll) grid = kNumCU * 64ll;
    if (vec4)
        hipLaunchKernelGGL((grad_gather_rows_kernel<NSRC, 4>), dim3(static_cast<unsigned>(grid)), dim3(block), 0, st, n, c, ld, col, cv,
                           rows_per_batch, target_rows, grad_out, weight, offsets, entries, grad_points);
    else
        hipLaunchKernelGGL((grad_gather_rows_kernel<NSRC, 1>), dim3(static_cast<unsigned>(grid)), dim3(block), 0, st, n, c, ld, col, cv,
                           rows_per_batch, target_rows, grad_out, weight, offsets, entries, grad_points);
    return launch_status();
}

}  // namespace hf
