// rcnn_batch.hip -- the hand-off between the two stages (hf/core/evaluator.py:963-983 save_rpn_features, hf/datasets/kitti/
// kitti_dataset.py:238-245 get_rpn_features, :473-487 the flip of the points).  The reference writes, and reads back, one
// (P, 5 + c) float32 row block per frame: [x, y, z, intensity, fg (0/1), rpn_fts...].  Two entry points move a batch of such
// blocks between that layout and the separate tensors the two models take:
//   pack    one thread per float4 of the packed rows (export side);
//   inputs  one thread per float4 of rpn_fts (load side), the thread that holds a row's first feature also writing its xyz
//           (x negated on flipped frames), intensity and fg flag.
// Layout: the row pitch W = 5 + c floats is only 4-byte aligned, but four rows are W float4s, so the packed buffer (16-byte
// aligned base) is a sequence of 4-row tiles of W float4s each.  Every output element has exactly one writer; no float is
// accumulated; the status bits are integer ORs.
#include "hf_common.h"

namespace hf {

constexpr int kHoMaxB = 1024, kHoMaxP = 1 << 20, kHoMaxC = 4096, kHoThreads = 256;
constexpr int kHoMaxBlocks = 1 << 20;   // grid-stride beyond this

__host__ __device__ inline bool ho_shape_ok(int b, int p, int c)
{
    return b >= 0 && b <= kHoMaxB && p >= 1 && p <= kHoMaxP && c >= 1 && c <= kHoMaxC;
}

// q / d for q < 2^53 and 1 <= d < 2^31 without the 64-bit integer division routine: the fp64 quotient, then one correction
__device__ __forceinline__ long long ho_div(long long q, int d)
{
    long long r = static_cast<long long>(static_cast<double>(q) / static_cast<double>(d));
    if (r * d > q) --r;
    else if ((r + 1) * d <= q) ++r;
    return r;
}

// ---------------------------------------------------------------- pack: (xyz, intensity, fg, rpn_fts) -> rows (b p, 5 + c)
__global__ __launch_bounds__(kHoThreads) void ho_pack_kernel(long long nrows, int c, const float *__restrict__ xyz,
                                                             const float *__restrict__ intensity,
                                                             const unsigned char *__restrict__ fg,
                                                             const float *__restrict__ fts, float *__restrict__ rows)
{
    const int w = 5 + c;
    const long long nvec = ho_div(nrows + 3, 4) * w;                 // float4s of the 4-row tiles
    const long long total = nrows * w;                               // floats of the buffer
    for (long long v = static_cast<long long>(blockIdx.x) * kHoThreads + threadIdx.x; v < nvec;
         v += static_cast<long long>(gridDim.x) * kHoThreads) {
        const long long tile = ho_div(v, w);
        int u = static_cast<int>(v - tile * w) * 4;                   // float offset inside the tile, < 4 w
        int r = u / w;
        int k = u - r * w;
        float val[4];
        for (int e = 0; e < 4; ++e) {
            const long long row = tile * 4 + r;
            float x = 0.0f;
            if (row < nrows) {
                if (k < 3) x = xyz[row * 3 + k];
                else if (k == 3) x = intensity[row];
                else if (k == 4) x = fg[row] ? 1.0f : 0.0f;
                else x = fts[row * c + (k - 5)];
            }
            val[e] = x;
            if (++k == w) { k = 0; ++r; }
        }
        const long long f0 = v * 4;
        if (f0 + 4 <= total) {
            *reinterpret_cast<float4 *>(rows + f0) = make_float4(val[0], val[1], val[2], val[3]);
        } else {
            for (int e = 0; e < 4; ++e)
                if (f0 + e < total) rows[f0 + e] = val[e];
        }
    }
}

// ---------------------------------------------------------------- inputs: rows (b, p, 5 + c) -> the model's tensors
__global__ __launch_bounds__(kHoThreads) void ho_inputs_kernel(int p, int c, long long nrows, const float *__restrict__ rows,
                                                               const int *__restrict__ flip, float *__restrict__ xyz,
                                                               float *__restrict__ intensity, unsigned char *__restrict__ fg,
                                                               float *__restrict__ fts, int *__restrict__ status)
{
    const int w = 5 + c;
    const long long total = nrows * c;                               // floats of rpn_fts
    const long long nvec = ho_div(total + 3, 4);
    for (long long v = static_cast<long long>(blockIdx.x) * kHoThreads + threadIdx.x; v < nvec;
         v += static_cast<long long>(gridDim.x) * kHoThreads) {
        const long long f0 = v * 4;
        long long row = ho_div(f0, c);
        int k = static_cast<int>(f0 - row * c);
        float val[4];
        for (int e = 0; e < 4; ++e) {
            float x = 0.0f;
            if (row < nrows) {
                const float *src = rows + row * w;
                x = src[5 + k];
                if (k == 0) {                                        // the row's own columns
                    const int f = static_cast<int>(ho_div(row, p));
                    const float sx = src[0];
                    xyz[row * 3 + 0] = flip[f] ? -sx : sx;
                    xyz[row * 3 + 1] = src[1];
                    xyz[row * 3 + 2] = src[2];
                    intensity[row] = src[3];
                    const float m = src[4];
                    fg[row] = m != 0.0f ? 1 : 0;
                    if (!(m == 0.0f || m == 1.0f)) atomicOr(status + f, HF_RCNN_BATCH_BAD_FG);
                }
            }
            val[e] = x;
            if (++k == c) { k = 0; ++row; }
        }
        if (f0 + 4 <= total) {
            *reinterpret_cast<float4 *>(fts + f0) = make_float4(val[0], val[1], val[2], val[3]);
        } else {
            for (int e = 0; e < 4; ++e)
                if (f0 + e < total) fts[f0 + e] = val[e];
        }
    }
}

inline int ho_grid(long long nvec)
{
    const long long blocks = (nvec + kHoThreads - 1) / kHoThreads;
    return static_cast<int>(blocks < kHoMaxBlocks ? (blocks > 0 ? blocks : 1) : kHoMaxBlocks);
}

}  // namespace hf

using namespace hf;

HF_API int hf_rpn_handoff_pack(int b, int p, int c, const float *xyz, const float *intensity, const unsigned char *fg_mask,
                               const float *rpn_fts, float *rows, hf_stream_t stream)
{
    if (!ho_shape_ok(b, p, c)) return HF_EINVAL;
    if (b == 0) return HF_OK;
    if (!xyz || !intensity || !fg_mask || !rpn_fts || !rows) return HF_EINVAL;
    if (reinterpret_cast<uintptr_t>(rows) & 15) return HF_EINVAL;      // the float4 stores
    const long long nrows = static_cast<long long>(b) * p;
    hipLaunchKernelGGL(ho_pack_kernel, dim3(ho_grid((nrows + 3) / 4 * (5 + c))), dim3(kHoThreads), 0, as_stream(stream), nrows, c,
                       xyz, intensity, fg_mask, rpn_fts, rows);
    return launch_status();
}

HF_API int hf_rcnn_batch_inputs(int b, int p, int c, const float *rows, const int *flip, float *xyz, float *intensity,
                                unsigned char *fg_mask, float *rpn_fts, int *status, hf_stream_t stream)
{
    if (!ho_shape_ok(b, p, c)) return HF_EINVAL;
    if (b == 0) return HF_OK;
    if (!rows || !flip || !xyz || !intensity || !fg_mask || !rpn_fts || !status) return HF_EINVAL;
    if (reinterpret_cast<uintptr_t>(rpn_fts) & 15) return HF_EINVAL;   // the float4 stores
    hipStream_t st = as_stream(stream);
    int e = hip_status(hipMemsetAsync(status, 0, sizeof(int) * static_cast<size_t>(b), st));
    if (e != HF_OK) return e;
    const long long nrows = static_cast<long long>(b) * p;
    hipLaunchKernelGGL(ho_inputs_kernel, dim3(ho_grid((nrows * c + 3) / 4)), dim3(kHoThreads), 0, st, p, c, nrows, rows, flip, xyz,
                       intensity, fg_mask, rpn_fts, status);
    return launch_status();
}
