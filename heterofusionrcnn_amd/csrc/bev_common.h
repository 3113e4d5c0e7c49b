// bev_common.h -- the rotated-BEV overlap helpers shared by bev_iou.hip (IoU matrix, oriented NMS) and rcnn_targets.hip
// (one thread per pair): points, the reference's segment / inside tests (bev_iou/bev_iou_g.cu), the per-box precompute
// and the two exact-zero-safe disjointness filters.  Everything evaluates in fp32 without contraction (-ffp-contract=off),
// so a pair gives the same bits in either file.
#pragma once

#include <math.h>

#include "hf_common.h"

namespace hf {

struct Pt { float x, y; };

constexpr float kIouEps = 1e-8f;  // bev_iou_g.cu:7

// bev_iou_g.cu:33-35
__device__ __forceinline__ float cross3(Pt p1, Pt p2, Pt p0)
{
    return (p1.x - p0.x) * (p2.y - p0.y) - (p2.x - p0.x) * (p1.y - p0.y);
}

// bev_iou_g.cu:62-91 (rect pre-check :37-43 inlined)
__device__ __forceinline__ bool seg_intersection(Pt p1, Pt p0, Pt q1, Pt q0, Pt &ans)
{
    const bool rect = fminf(p0.x, p1.x) <= fmaxf(q0.x, q1.x) && fminf(q0.x, q1.x) <= fmaxf(p0.x, p1.x) &&
                      fminf(p0.y, p1.y) <= fmaxf(q0.y, q1.y) && fminf(q0.y, q1.y) <= fmaxf(p0.y, p1.y);
    if (!rect) return false;
    const float s1 = cross3(q0, p1, p0);
    const float s2 = cross3(p1, q1, p0);
    const float s3 = cross3(p0, q1, q0);
    const float s4 = cross3(q1, p1, q0);
    if (!(s1 * s2 > 0 && s3 * s4 > 0)) return false;
    const float s5 = cross3(q1, p1, p0);
    if (fabsf(s5 - s1) > kIouEps) {
        ans.x = (s5 * q0.x - s1 * q1.x) / (s5 - s1);
        ans.y = (s5 * q0.y - s1 * q1.y) / (s5 - s1);
    } else {
        const float a0 = p0.y - p1.y, b0 = p1.x - p0.x, c0 = p0.x * p1.y - p1.x * p0.y;
        const float a1 = q0.y - q1.y, b1 = q1.x - q0.x, c1 = q0.x * q1.y - q1.x * q0.y;
        const float D = a0 * b1 - a1 * b0;
        ans.x = (b0 * c1 - b1 * c0) / D;
        ans.y = (a1 * c0 - a0 * c1) / D;
    }
    return true;
}

// check_in_box2d, bev_iou_g.cu:45-60, with cos(-a)=ac, sin(-a)=-as passed in
__device__ __forceinline__ bool in_box2d(const float *box, float ac, float as_neg, Pt p)
{
    const float MARGIN = 1e-5f;
    const float cx = (box[0] + box[2]) / 2, cy = (box[1] + box[3]) / 2;
    const float rx = (p.x - cx) * ac + (p.y - cy) * as_neg + cx;
    const float ry = -(p.x - cx) * as_neg + (p.y - cy) * ac + cy;
    return rx > box[0] - MARGIN && rx < box[2] + MARGIN && ry > box[1] - MARGIN && ry < box[3] + MARGIN;
}

// iou_bev(box_a, box_b, s_overlap), bev_iou_g.cu:208-215, for two [x1, y1, x2, y2, angle] boxes
__device__ __forceinline__ float iou_from_overlap(const float *a, const float *b, float s)
{
    const float sa = (a[2] - a[0]) * (a[3] - a[1]);
    const float sb = (b[2] - b[0]) * (b[3] - b[1]);
    return s / fmaxf(sa + sb - s, kIouEps);
}

// rotate_around_center, bev_iou_g.cu:92-96
__device__ __forceinline__ Pt rot_center(Pt c, float ac, float as, Pt p)
{
    Pt r;
    r.x = (p.x - c.x) * ac + (p.y - c.y) * as + c.x;
    r.y = -(p.x - c.x) * as + (p.y - c.y) * ac + c.y;
    return r;
}

// Everything about one box that does not depend on its partner: evaluated once per box per tile
// (the reference recomputes cos/sin and the rotated corners for every pair, bev_iou_g.cu:130-140).
struct __attribute__((aligned(16))) BoxPre {
    float cx, cy, rad, mag; // centre, the circumradius (half diagonal), |cx| + |cy| + rad: the first filter
                            // reads these four with one 16-byte LDS access
    Pt cor[4];              // rotated corners, order of bev_iou_g.cu:118-128
    float cs, sn;           // cos(angle), sin(angle)
    float box[5];           // x1, y1, x2, y2, angle
    float pad_;
};

static_assert(sizeof(BoxPre) == 80, "the NMS workspace table and its 16-byte copies assume 80 bytes per box");

__device__ __forceinline__ void box_precompute(const float *b, BoxPre &o)
{
#pragma unroll
    for (int d = 0; d < 5; ++d) o.box[d] = b[d];
    const Pt c = { (b[0] + b[2]) / 2, (b[1] + b[3]) / 2 };
    o.cs = cosf(b[4]);
    o.sn = sinf(b[4]);
    o.cor[0] = rot_center(c, o.cs, o.sn, Pt{ b[0], b[1] });
    o.cor[1] = rot_center(c, o.cs, o.sn, Pt{ b[2], b[1] });
    o.cor[2] = rot_center(c, o.cs, o.sn, Pt{ b[2], b[3] });
    o.cor[3] = rot_center(c, o.cs, o.sn, Pt{ b[0], b[3] });
    o.cx = c.x;
    o.cy = c.y;
    // half the diagonal: the distance from the centre to every rotated corner (rotation keeps it; its fp32 rounding is covered
    // by the filters' slack of 1e-3 + 1e-5 * mag).  Round 4: was the half perimeter (w + h) / 2, which is 30 % longer for a
    // 3.9 x 1.6 box -- 1.7 x as many pairs survived the circle filter and went through the separating-axis test
    const float bw = b[2] - b[0], bh = b[3] - b[1];
    o.rad = 0.5f * sqrtf(bw * bw + bh * bh) * 1.000001f;
    o.mag = fabsf(o.cx) + fabsf(o.cy) + o.rad;
}

// first filter, 6 LDS words per pair: centres further apart than the two radius bounds plus a slack that
// dwarfs MARGIN = 1e-5 and fp32 rounding.  true => the reference computes exactly 0 (no edge crossing, no
// corner inside: bev_iou_g.cu:150-176 leave cnt = 0).
__device__ __forceinline__ bool circles_apart(const BoxPre &a, const BoxPre &b)
{
    const float mag = a.mag + b.mag;
    const float reach = a.rad + b.rad + 1e-3f + 1e-5f * mag;
    const float dx = a.cx - b.cx, dy = a.cy - b.cy;
    return dx * dx + dy * dy > reach * reach;  // NaN/inf compare false -> next filter
}

// second filter (survivors of the first only): separating-axis test over the four edge directions of the
// rotated corners, accepted only when the gap along some axis exceeds the same kind of slack.
__device__ __forceinline__ bool surely_disjoint(const BoxPre &a, const BoxPre &b)
{
    float mag = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        mag = fmaxf(mag, fmaxf(fmaxf(fabsf(a.cor[k].x), fabsf(a.cor[k].y)), fmaxf(fabsf(b.cor[k].x), fabsf(b.cor[k].y))));
    const float slack = 1e-3f + 1e-5f * mag;
    bool sep = false;
#pragma unroll
    for (int which = 0; which < 2; ++which) {
        const BoxPre &p = which == 0 ? a : b;
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            // axis = edge direction cor[e+1] - cor[e] (not normalised; gaps are compared scaled by its length)
            const float ux = p.cor[e + 1].x - p.cor[e].x, uy = p.cor[e + 1].y - p.cor[e].y;
            const float len = fabsf(ux) + fabsf(uy);  // >= |u|: makes the required gap larger, never smaller
            float amin = INFINITY, amax = -INFINITY, bmin = INFINITY, bmax = -INFINITY;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float pa = a.cor[k].x * ux + a.cor[k].y * uy;
                const float pb = b.cor[k].x * ux + b.cor[k].y * uy;
                amin = fminf(amin, pa); amax = fmaxf(amax, pa);
                bmin = fminf(bmin, pb); bmax = fmaxf(bmax, pb);
            }
            const float gap = fmaxf(bmin - amax, amin - bmax);
            if (gap > (slack + 4e-6f * mag) * len && len > 0.f) sep = true;  // projections round at ~mag*|u|*1e-6
        }
    }
    return sep;  // NaN / inf inputs compare false -> full path
}

}  // namespace hf
