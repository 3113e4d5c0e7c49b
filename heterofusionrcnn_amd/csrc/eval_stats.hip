// eval_stats.hip -- the statistics stage of checkpoint validation (hf/core/evaluator.py:149-377 run_checkpoint_once) on the device.
//
// hf_proposal_stats   compute_iou.box3d_iou_tf, then box_util.compute_recall_iou (hf/core/box_util.py:131-174), per frame, and the
//                     per-frame sums evaluator.py:984-1064 accumulates.  Two launches:
//   pairs   one thread per (proposal, GT) pair, 256 pairs per workgroup, grid (pair tiles, frames): the pair is clipped ONCE
//           (box3d_iou_pair, box3d_common.h: the device function of hf_box3d_iou_matrix; a pair whose bounding circles are apart
//           costs no clip) and both the 3D IoU and the BEV IoU are formed from that overlap; zeros in the padding;
//   reduce  one 256-thread workgroup per frame over the two matrices: a group of W = min(64, pow2 >= g) lanes per proposal row
//           (max and FIRST argmax of the 3D row, max of the BEV row, butterfly shuffles inside the group), one thread per GT column
//           and row parity (column maximum -> recalled at 0.5 / 0.7, counted with wave ballots), then the three sums in fp64:
//           thread t adds rows t, t + 256 in ascending order, a fixed butterfly inside the wave, the four waves in order.
// No floating-point atomic anywhere: two calls give the same bits.
// Deviation from the reference: a frame without GT contributes 0 to the angle sum (the reference adds sum |ry| against an
// all-zero box, evaluator.py:1040-1050).
//
// hf_argmax_accuracy  calculate_cls_accuracy (evaluator.py:917-932) as counts: rows whose first argmax equals max(target, 0), per
//                     group of consecutive rows.  A memset node and one launch: ballots per wave, one integer atomic per workgroup.
#include <limits.h>
#include <math.h>

#include "bev_common.h"
#include "box3d_common.h"
#include "hf_common.h"

namespace hf {

constexpr int kStatMaxB = 1024, kStatMaxM = 512, kStatMaxG = 128, kStatThreads = 256;   // the limits of hf_box3d_iou_matrix
constexpr int kAccThreads = 256, kAccRowsPerThread = 4, kAccMaxC = 8;

__host__ __device__ inline size_t stat_align(size_t v) { return (v + 255) & ~static_cast<size_t>(255); }
__host__ __device__ inline size_t stat_matrix_bytes(int b, int m, int g) { return stat_align(sizeof(float) * static_cast<size_t>(b) * m * g); }

struct StatArgs {
    int b, m, g, w;               // w: lanes per proposal row in the reduction, a power of two <= 64
    const float *proposals;       // (b, m, 7)
    const int *pcount, *gcount;   // (b)
    const float *gt;              // (b, g, 8)
    float *m3, *m2;               // (b, m, g): the caller's iou3d / iou2d, or the workspace
    float *best3, *best2;         // (b, m)
    int *best_gt;                 // (b, m)
    int *counts;                  // (b, 4)
    double *sums;                 // (b, 3)
};

__global__ __launch_bounds__(256) void proposal_pairs_kernel(StatArgs a)
{
    const int f = blockIdx.y;
    const int p = blockIdx.x * 256 + threadIdx.x;
    const int per_frame = a.m * a.g;   // <= 65 536
    if (p >= per_frame) return;
    const int i = p / a.g, j = p - i * a.g;
    float v3 = 0.0f, v2 = 0.0f;
    if (i < a.pcount[f] && j < a.gcount[f])
        v3 = box3d_iou_pair(a.proposals + (static_cast<long long>(f) * a.m + i) * 7, a.gt + (static_cast<long long>(f) * a.g + j) * 8, &v2);
    const long long o = static_cast<long long>(f) * per_frame + p;
    a.m3[o] = v3;
    a.m2[o] = v2;
}

__global__ __launch_bounds__(kStatThreads) void proposal_reduce_kernel(StatArgs a)
{
    __shared__ float s_b2[kStatMaxM], s_b3[kStatMaxM], s_ang[kStatMaxM];
    __shared__ float s_col[2][kStatMaxG];
    __shared__ int s_hit[2][2];
    __shared__ double s_part[kStatThreads / 64][3];
    const int f = blockIdx.x, t = threadIdx.x;
    const int n = min(max(a.pcount[f], 0), a.m), ng = min(max(a.gcount[f], 0), a.g);
    const long long frame = static_cast<long long>(f) * a.m * a.g;   // g == 0: the matrices are never read
    const float *iou3 = a.m3 + frame, *iou2 = a.m2 + frame;
    // ---- per proposal: row maxima and the first argmax of the 3D row (np.argmax: an all-zero row gives column 0)
    {
        const int w = a.w, sub = t & (w - 1), grp = t / w, groups = kStatThreads / w;
        for (int i0 = 0; i0 < a.m; i0 += groups) {   // uniform trip count: every lane takes part in the shuffles
            const int i = i0 + grp;
            const bool live = i < n && ng > 0;
            float v3 = -1.0f, v2 = -1.0f;
            int am = INT_MAX;
            if (live)
                for (int j = sub; j < ng; j += w) {
                    const float c3 = iou3[i * a.g + j], c2 = iou2[i * a.g + j];
                    if (c3 > v3) { v3 = c3; am = j; }
                    v2 = fmaxf(v2, c2);
                }
            for (int off = w >> 1; off > 0; off >>= 1) {
                const float o3 = __shfl_xor(v3, off, 64), o2 = __shfl_xor(v2, off, 64);
                const int oa = __shfl_xor(am, off, 64);
                if (o3 > v3 || (o3 == v3 && oa < am)) { v3 = o3; am = oa; }
                v2 = fmaxf(v2, o2);
            }
            if (sub == 0 && i < a.m) {
                float ang = 0.0f;
                if (live) {
                    ang = fabsf(a.proposals[(static_cast<long long>(f) * a.m + i) * 7 + 6] - a.gt[(static_cast<long long>(f) * a.g + am) * 8 + 6]);
                } else {
                    v3 = 0.0f; v2 = 0.0f; am = -1;
                }
                const long long o = static_cast<long long>(f) * a.m + i;
                a.best3[o] = v3; a.best2[o] = v2; a.best_gt[o] = am;
                s_b3[i] = v3; s_b2[i] = v2; s_ang[i] = ang;
            }
        }
    }
    // ---- per GT: column maximum over the valid proposals, rows of one parity per thread
    {
        const int j = t & (kStatMaxG - 1), h = t >> 7;
        float cm = 0.0f;
        if (j < ng)
            for (int i = h; i < n; i += 2) cm = fmaxf(cm, iou3[i * a.g + j]);
        s_col[h][j] = cm;
    }
    __syncthreads();
    if (t < kStatMaxG) {   // waves 0 and 1, whole
        const float cm = fmaxf(s_col[0][t], s_col[1][t]);
        const unsigned long long b50 = __ballot(t < ng && cm > 0.5f), b70 = __ballot(t < ng && cm > 0.7f);   // strict, as the reference
        if ((t & 63) == 0) { s_hit[t >> 6][0] = __popcll(b50); s_hit[t >> 6][1] = __popcll(b70); }
    }
    // ---- the three sums in fp64, a fixed order
    {
        double d[3] = { 0.0, 0.0, 0.0 };
        for (int i = t; i < n; i += kStatThreads) {
            d[0] += static_cast<double>(s_b2[i]); d[1] += static_cast<double>(s_b3[i]); d[2] += static_cast<double>(s_ang[i]);
        }
#pragma unroll
        for (int k = 0; k < 3; ++k)
            for (int off = 32; off > 0; off >>= 1) d[k] += __shfl_xor(d[k], off, 64);
        if ((t & 63) == 0)
            for (int k = 0; k < 3; ++k) s_part[t >> 6][k] = d[k];
    }
    __syncthreads();
    if (t < 3) {
        double s = s_part[0][t];
        for (int wv = 1; wv < kStatThreads / 64; ++wv) s += s_part[wv][t];
        a.sums[3 * f + t] = s;
    }
    if (t == 0) {
        int *c = a.counts + 4 * f;
        c[0] = n; c[1] = ng; c[2] = s_hit[0][0] + s_hit[1][0]; c[3] = s_hit[0][1] + s_hit[1][1];
    }
}

// one workgroup per (group, chunk of kAccThreads * kAccRowsPerThread rows); correct[] was cleared on the stream before
__global__ __launch_bounds__(kAccThreads) void argmax_accuracy_kernel(long long rows_per_group, int c, int chunks,
                                                                      const float *__restrict__ logits, const int *__restrict__ target,
                                                                      int *__restrict__ correct)
{
    __shared__ int s_hits[kAccThreads / 64];
    const int t = threadIdx.x;
    const int grp = blockIdx.x / chunks, chunk = blockIdx.x - grp * chunks;
    const long long base = static_cast<long long>(grp) * rows_per_group;
    int hits = 0;
#pragma unroll
    for (int k = 0; k < kAccRowsPerThread; ++k) {
        const long long r = static_cast<long long>(chunk) * (kAccThreads * kAccRowsPerThread) + k * kAccThreads + t;
        bool hit = false;
        if (r < rows_per_group) {
            const float *l = logits + (base + r) * c;
            float best = l[0];
            int am = 0;
            for (int q = 1; q < c; ++q) {
                const float v = l[q];
                if (v > best) { best = v; am = q; }   // first maximum, as np.argmax
            }
            hit = am == max(target[base + r], 0);     // a negative target: the all-zero one-hot row, argmax 0
        }
        hits += __popcll(__ballot(hit));              // wave-uniform
    }
    if ((t & 63) == 0) s_hits[t >> 6] = hits;
    __syncthreads();
    if (t == 0) {
        int total = 0;
        for (int wv = 0; wv < kAccThreads / 64; ++wv) total += s_hits[wv];
        if (total) atomicAdd(&correct[grp], total);
    }
}

inline bool stat_limits_ok(int b, int m, int g) { return b >= 0 && b <= kStatMaxB && m >= 1 && m <= kStatMaxM && g >= 0 && g <= kStatMaxG; }

}  // namespace hf

using namespace hf;

HF_API size_t hf_proposal_stats_workspace(int b, int m, int g)
{
    if (!stat_limits_ok(b, m, g)) return 0;
    return 2 * stat_matrix_bytes(b, m, g);
}

HF_API int hf_proposal_stats(int b, int m, int g, const float *proposals, const int *proposal_count, const float *gt, const int *gt_count,
                             float *iou3d, float *iou2d, float *best_iou3d, float *best_iou2d, int *best_gt, int *counts, double *sums,
                             void *workspace, size_t workspace_bytes, hf_stream_t stream)
{
    if (!stat_limits_ok(b, m, g)) return HF_EINVAL;
    if (b == 0) return HF_OK;
    if (!proposals || !proposal_count || !gt_count || (g > 0 && !gt) || !best_iou3d || !best_iou2d || !best_gt || !counts || !sums)
        return HF_EINVAL;
    const size_t need = 2 * stat_matrix_bytes(b, m, g);
    if (need > 0 && (!workspace || workspace_bytes < need)) return HF_EWORKSPACE;
    unsigned char *ws = static_cast<unsigned char *>(workspace);
    StatArgs a;
    a.b = b; a.m = m; a.g = g;
    a.w = 1;
    while (a.w < g && a.w < 64) a.w <<= 1;
    a.proposals = proposals; a.pcount = proposal_count; a.gcount = gt_count; a.gt = gt;
    a.m3 = iou3d ? iou3d : reinterpret_cast<float *>(ws);
    a.m2 = iou2d ? iou2d : reinterpret_cast<float *>(ws + stat_matrix_bytes(b, m, g));
    a.best3 = best_iou3d; a.best2 = best_iou2d; a.best_gt = best_gt; a.counts = counts; a.sums = sums;
    hipStream_t st = as_stream(stream);
    if (g > 0) hipLaunchKernelGGL(proposal_pairs_kernel, dim3(div_up(static_cast<long long>(m) * g, 256), b), dim3(256), 0, st, a);
    hipLaunchKernelGGL(proposal_reduce_kernel, dim3(b), dim3(kStatThreads), 0, st, a);
    return launch_status();
}

HF_API int hf_argmax_accuracy(long long rows, int c, int groups, const float *logits, const int *target, int *correct, hf_stream_t stream)
{
    if (rows < 0 || c < 2 || c > kAccMaxC || groups < 1 || rows % groups != 0) return HF_EINVAL;
    if (!correct || (rows > 0 && (!logits || !target))) return HF_EINVAL;
    const long long rows_per_group = rows / groups;
    const long long chunks = (rows_per_group + kAccThreads * kAccRowsPerThread - 1) / (kAccThreads * kAccRowsPerThread);
    if (chunks * groups > INT_MAX) return HF_EINVAL;
    hipStream_t st = as_stream(stream);
    const int cleared = hip_status(hipMemsetAsync(correct, 0, sizeof(int) * static_cast<size_t>(groups), st));
    if (cleared != HF_OK || rows == 0) return cleared;
    hipLaunchKernelGGL(argmax_accuracy_kernel, dim3(static_cast<unsigned>(chunks * groups)), dim3(kAccThreads), 0, st, rows_per_group, c,
                       static_cast<int>(chunks), logits, target, correct);
    return launch_status();
}
