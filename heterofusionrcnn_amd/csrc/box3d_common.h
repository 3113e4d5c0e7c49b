// box3d_common.h -- the one-thread rotated overlap and the 3D IoU of one box pair, shared by rcnn_targets.hip (target layer,
// hf_box3d_iou_matrix) and eval_stats.hip (hf_proposal_stats): one definition, so a pair gives the same bits in every kernel.
#pragma once

#include <math.h>

#include "bev_common.h"
#include "hf_common.h"

namespace hf {

// ---------------------------------------------------------------- one-thread rotated overlap
// box_overlap (bev_iou_g.cu:102-206) with the candidate points in the reference's order: the 16 edge crossings (i, j), then
// per corner k "B[k] inside A", "A[k] inside B"; centroid in that order, atan2 of each point, the stable sort's positions
// (rank = smaller angle, or equal angle and earlier point), the fan summed in rank order.  box_overlap_group in bev_iou.hip
// evaluates the same operations on eight lanes, so a pair gives the same overlap in both files.
__device__ inline float box_overlap_serial(const BoxPre &pa, const BoxPre &pb)
{
    float px[24], py[24], ang[24];
    int order[24];
    int cnt = 0;
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            Pt x;
            if (seg_intersection(pa.cor[(i + 1) & 3], pa.cor[i], pb.cor[(j + 1) & 3], pb.cor[j], x)) {
                px[cnt] = x.x; py[cnt] = x.y; ++cnt;
            }
        }
    for (int k = 0; k < 4; ++k) {
        if (in_box2d(pa.box, pa.cs, -pa.sn, pb.cor[k])) { px[cnt] = pb.cor[k].x; py[cnt] = pb.cor[k].y; ++cnt; }
        if (in_box2d(pb.box, pb.cs, -pb.sn, pa.cor[k])) { px[cnt] = pa.cor[k].x; py[cnt] = pa.cor[k].y; ++cnt; }
    }
    if (cnt < 3) return 0.0f;
    Pt ctr = { 0.f, 0.f };
    for (int k = 0; k < cnt; ++k) { ctr.x = ctr.x + px[k]; ctr.y = ctr.y + py[k]; }
    ctr.x /= cnt;
    ctr.y /= cnt;
    for (int k = 0; k < cnt; ++k) ang[k] = atan2f(py[k] - ctr.y, px[k] - ctr.x);
    for (int k = 0; k < cnt; ++k) order[k] = 0;   // NaN angles can share a rank: every slot read below stays in range
    for (int k = 0; k < cnt; ++k) {
        int rk = 0;
        for (int o = 0; o < cnt; ++o) rk += (ang[o] < ang[k] || (ang[o] == ang[k] && o < k)) ? 1 : 0;
        order[rk] = k;
    }
    const float x0 = px[order[0]], y0 = py[order[0]];
    float area = 0.f;
    for (int r = 1; r <= cnt - 2; ++r) {
        const float ux = px[order[r]] - x0, uy = py[order[r]] - y0;
        const float vx = px[order[r + 1]] - x0, vy = py[order[r + 1]] - y0;
        area += ux * vy - uy * vx;
    }
    return fabsf(area) / 2.0f;
}

// modules.box3d_iou for one pair of [x, y, z, l, w, h, ry] boxes (y is the bottom, camera y down): boxes3d_to_bev, the BEV
// overlap, clamp(min(a_max, b_max) - max(a_min, b_min), 0), overlap / clamp(vol_a + vol_b - overlap, 1e-7).  bev_iou (may be
// NULL) receives the BEV IoU of the same pair from the SAME overlap: iou_bev of the two boxes3d_to_bev rows, what
// hf_compute_bev_iou returns for them.
__device__ inline float box3d_iou_pair(const float *a, const float *b, float *bev_iou)
{
    float ea[5], eb[5];
    {
        const float hl = a[3] / 2, hw = a[4] / 2;
        ea[0] = a[0] - hl; ea[1] = a[2] - hw; ea[2] = a[0] + hl; ea[3] = a[2] + hw; ea[4] = a[6];
    }
    {
        const float hl = b[3] / 2, hw = b[4] / 2;
        eb[0] = b[0] - hl; eb[1] = b[2] - hw; eb[2] = b[0] + hl; eb[3] = b[2] + hw; eb[4] = b[6];
    }
    BoxPre pa, pb;
    box_precompute(ea, pa);
    box_precompute(eb, pb);
    const float bev = circles_apart(pa, pb) ? 0.0f : box_overlap_serial(pa, pb);   // far pairs are exactly 0 (bev_common.h)
    if (bev_iou) *bev_iou = iou_from_overlap(ea, eb, bev);
    const float oh = fmaxf(fminf(a[1], b[1]) - fmaxf(a[1] - a[5], b[1] - b[5]), 0.0f);
    const float o3 = bev * oh;
    const float va = a[3] * a[4] * a[5], vb = b[3] * b[4] * b[5];
    return o3 / fmaxf(va + vb - o3, 1e-7f);
}

__device__ inline float box3d_iou_dev(const float *a, const float *b) { return box3d_iou_pair(a, b, nullptr); }

}  // namespace hf
