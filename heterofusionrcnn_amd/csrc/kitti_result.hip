// kitti_result.hip -- the image rectangle and the keep flag of every detection of a batch, the per-box host loop of the
// result writer (hf/core/evaluator_utils.py:88-166, box_3d_projector.py:88-163; inference.write_frame_results and
// project_box3d_to_image) as ONE launch, one thread per detection, in fp64 and in the host code's operation order:
//   corners    compute_box_corners_3d: x = (c xs + s zs) + x, y = ys + y, z = (-s xs + c zs) + z, c / s = cos / sin of double(ry),
//              xs = +-l/2, zs = +-w/2, ys = 0 / -h, in the reference's corner order;
//   project    [x y z 1] . P2^T added left to right, u / w and v / w;
//   rectangle  min / max over the eight corners (a NaN propagates, as np.min / np.max propagate it);
//   reject     the rectangle lies outside the image, or is wider / taller than 0.8 of it;
//   truncate   to [0, w] x [0, h] with Python's max / min (a NaN first operand stays).
// keep = not rejected and score >= score_min (fp32 against fp32, as NumPy compares a float32 array with a Python float).
// Every output element has one writer; nothing is accumulated across threads; -ffp-contract=off keeps the operations apart.
#include <math.h>

#include "hf_common.h"

namespace hf {

namespace {

constexpr int kResThreads = 256;
constexpr int kResMaxBlocks = 1 << 20;   // grid-stride beyond this

// np.min / np.max over a run: the first NaN met stays
__device__ inline double np_min(double m, double v) { return (v < m || v != v) ? v : m; }
__device__ inline double np_max(double m, double v) { return (v > m || v != v) ? v : m; }

__global__ void __launch_bounds__(kResThreads) k_result_boxes(int b, long long n, const float *__restrict__ boxes3d,
                                                              const float *__restrict__ scores, const int *__restrict__ frame,
                                                              const double *__restrict__ p2, const int *__restrict__ image_wh,
                                                              float score_min, double *__restrict__ boxes2d,
                                                              unsigned char *__restrict__ keep)
{
    for (long long i = static_cast<long long>(blockIdx.x) * kResThreads + threadIdx.x; i < n;
         i += static_cast<long long>(gridDim.x) * kResThreads) {
        double *out = boxes2d + i * 4;
        const int f = frame[i];
        if (f < 0 || f >= b) {                                   // no frame to project into: never kept
            out[0] = 0.0; out[1] = 0.0; out[2] = 0.0; out[3] = 0.0;
            keep[i] = 0;
            continue;
        }
        const float *bx = boxes3d + i * 7;
        const double x = bx[0], y = bx[1], z = bx[2], l = bx[3], w = bx[4], h = bx[5], ry = bx[6];
        const double c = cos(ry), s = sin(ry);
        const double hl = l / 2, hw = w / 2;
        const double xs[8] = { hl, hl, -hl, -hl, hl, hl, -hl, -hl };
        const double zs[8] = { hw, -hw, -hw, hw, hw, -hw, -hw, hw };
        const double ys[8] = { 0.0, 0.0, 0.0, 0.0, -h, -h, -h, -h };
        const double *p = p2 + static_cast<long long>(f) * 12;
        double u0 = 0.0, v0 = 0.0, u1 = 0.0, v1 = 0.0;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const double cx = c * xs[k] + s * zs[k] + x;
            const double cy = ys[k] + y;
            const double cz = -s * xs[k] + c * zs[k] + z;
            const double pu = cx * p[0] + cy * p[1] + cz * p[2] + p[3];
            const double pv = cx * p[4] + cy * p[5] + cz * p[6] + p[7];
            const double pw = cx * p[8] + cy * p[9] + cz * p[10] + p[11];
            const double u = pu / pw, v = pv / pw;
            if (k == 0) {
                u0 = u1 = u;
                v0 = v1 = v;
            } else {
                u0 = np_min(u0, u); u1 = np_max(u1, u);
                v0 = np_min(v0, v); v1 = np_max(v1, v);
            }
        }
        const double iw = static_cast<double>(image_wh[2 * f]), ih = static_cast<double>(image_wh[2 * f + 1]);
        bool rejected = u0 > iw || v0 > ih || u1 < 0.0 || v1 < 0.0;
        rejected = rejected || u1 - u0 > 0.8 * iw || v1 - v0 > 0.8 * ih;
        out[0] = 0.0 > u0 ? 0.0 : u0;                            // max(box[0], 0)
        out[1] = 0.0 > v0 ? 0.0 : v0;
        out[2] = iw < u1 ? iw : u1;                              // min(box[2], w)
        out[3] = ih < v1 ? ih : v1;
        keep[i] = (!rejected && scores[i] >= score_min) ? 1 : 0;
    }
}

}  // namespace

}  // namespace hf

using namespace hf;

HF_API int hf_kitti_result_boxes(int b, long long n, const float *boxes3d, const float *scores, const int *frame, const double *p2,
                                 const int *image_wh, float score_min, double *boxes2d, unsigned char *keep, hf_stream_t stream)
{
    if (b <= 0 || n < 0) return HF_EINVAL;
    if (n == 0) return HF_OK;
    if (!boxes3d || !scores || !frame || !p2 || !image_wh || !boxes2d || !keep) return HF_EINVAL;
    const long long blocks = (n + kResThreads - 1) / kResThreads;
    hipLaunchKernelGGL(k_result_boxes, dim3(static_cast<unsigned>(blocks < kResMaxBlocks ? blocks : kResMaxBlocks)), dim3(kResThreads),
                       0, as_stream(stream), b, n, boxes3d, scores, frame, p2, image_wh, score_min, boxes2d, keep);
    return launch_status();
}
