// kitti_eval.hip -- the KITTI object evaluator (2D / BEV / 3D AP) on the device: the counting rules of the reference's
// scripts/offline_eval/kitti_native_eval/evaluate_object_3d_offline.cpp (restated in include/hfops.h and DESIGN.md §8).
// The reference re-clips every detection x ground-truth polygon pair inside every matching pass; here the overlaps are
// computed once, in fp64, and every matching pass reads them.  Six launches, no host synchronisation:
//   overlaps    one thread per (frame, det, gt) pair: image IoU, BEV and 3D IoU (fp64 Sutherland-Hodgman clip of the two
//               rotated rectangles), and the criterion-0 forms (intersection over the detection) used against DontCare rows;
//   pass1       one thread per (list, frame), list = (metric, class, difficulty): the recall pass without false positives,
//               its TP scores into the frame's slots of the list (padding -inf) and the frame's count of valid GTs;
//   merge       log2(#GT rows) launches of a stable descending merge sort of every list's scores (one thread per element,
//               its output position from a binary search in the other run);
//   thresholds  one workgroup per list: the ranks getThresholds selects (a binary search per recall step, see below);
//   pass2       one workgroup per frame, a lane per (list, threshold) task: TP / FP / FN and the orientation similarity sum;
//   finalize    one workgroup per list, a lane per threshold: the frame sums in frame order, precision, aos, aos_ground and the
//               suffix maximum with std::max_element semantics.
// Integer counts are exact; the similarity sums are added in the reference's order (per frame in GT order, then frames in
// order), so results are bit-identical from run to run (no float atomics anywhere).
#include <limits.h>
#include <math.h>

#include "hf_common.h"

namespace hf {

namespace {

constexpr int kLists = 27, kSteps = 41, kTasks = kLists * kSteps;
constexpr int kCols = HF_KITTI_COLS;
constexpr int kMaxPoly = 16;                     // Sutherland-Hodgman output capacity (8 suffice for two rectangles)
constexpr int kMaskWords = HF_KITTI_MAX_DET / 32;
constexpr int kThreads = 256;
constexpr double kNoDetection = -10000000.0;
enum { C_X1, C_Y1, C_X2, C_Y2, C_ALPHA, C_H, C_W, C_L, C_T1, C_T2, C_T3, C_RY, C_EXTRA };

__device__ inline int min_height(int d) { return d == 0 ? 40 : 25; }
__device__ inline double max_truncation(int d) { return d == 0 ? 0.15 : (d == 1 ? 0.3 : 0.5); }

// std::max / std::min (NaN operands resolve as they do there)
__device__ inline double smax(double a, double b) { return (a < b) ? b : a; }
__device__ inline double smin(double a, double b) { return (b < a) ? b : a; }

// ------------------------------------------------------------------------------------------------ overlaps (fp64)

// toPolygon: corners (l/2, w/2), (l/2, -w/2), (-l/2, -w/2), (-l/2, w/2) through [[cos, sin], [-sin, cos]], then + (t1, t3)
__device__ void bev_quad(const double *r, double *x, double *z)
{
    const double c = cos(r[C_RY]), s = sin(r[C_RY]);
    const double hl = r[C_L] / 2, hw = r[C_W] / 2;
    const double cx[4] = { hl, hl, -hl, -hl }, cz[4] = { hw, -hw, -hw, hw };
    for (int i = 0; i < 4; ++i) {
        x[i] = c * cx[i] + s * cz[i] + r[C_T1];
        z[i] = -s * cx[i] + c * cz[i] + r[C_T3];
    }
}

// twice the signed (shoelace) area
__device__ double area2(const double *x, const double *z, int n)
{
    double a = 0.0;
    for (int k = 0; k < n; ++k) {
        const int k1 = (k + 1 == n) ? 0 : k + 1;
        a += x[k] * z[k1] - x[k1] * z[k];
    }
    return a;
}

// area of (subject quad) ∩ (clip quad): the subject clipped by the clip quad's four edge half-planes, inside = on the
// clip quad's side of the edge (either winding), boundary included
__device__ double quad_intersection(const double *sx, const double *sz, double sa2, const double *cx, const double *cz, double ca2)
{
    if (!(fabs(sa2) > 0.0) || !(fabs(ca2) > 0.0)) return 0.0;
    const double o = ca2 > 0.0 ? 1.0 : -1.0;
    double px[kMaxPoly], pz[kMaxPoly], qx[kMaxPoly], qz[kMaxPoly];
    int n = 4;
    for (int k = 0; k < 4; ++k) { px[k] = sx[k]; pz[k] = sz[k]; }
    for (int e = 0; e < 4 && n > 0; ++e) {
        const int e1 = (e + 1) & 3;
        const double ex = cx[e], ez = cz[e], dx = cx[e1] - cx[e], dz = cz[e1] - cz[e];
        int m = 0;
        for (int k = 0; k < n; ++k) {
            const int k1 = (k + 1 == n) ? 0 : k + 1;
            const double dp = o * (dx * (pz[k] - ez) - dz * (px[k] - ex));
            const double dq = o * (dx * (pz[k1] - ez) - dz * (px[k1] - ex));
            const bool pin = dp >= 0.0, qin = dq >= 0.0;
            if (pin != qin && m < kMaxPoly) {
                const double t = dp / (dp - dq);
                qx[m] = px[k] + (px[k1] - px[k]) * t;
                qz[m] = pz[k] + (pz[k1] - pz[k]) * t;
                ++m;
            }
            if (qin && m < kMaxPoly) { qx[m] = px[k1]; qz[m] = pz[k1]; ++m; }
        }
        n = m;
        for (int k = 0; k < n; ++k) { px[k] = qx[k]; pz[k] = qz[k]; }
    }
    if (n < 3) return 0.0;
    return fabs(area2(px, pz, n)) / 2;
}

// one thread per pair p = pair_off[f] + g * n_det(f) + d -> ov[p] = { image, BEV, 3D, image c0, BEV c0, 3D c0 }
__global__ void __launch_bounds__(kThreads) k_overlaps(int frames, const long long *gt_off, const long long *det_off,
                                                       const long long *pair_off, long long n_pairs, const double *gt,
                                                       const double *det, double *ov)
{
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_pairs) return;
    int lo = 0, hi = frames - 1;                              // the last frame whose pairs start at or before p
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (pair_off[mid] <= p) lo = mid; else hi = mid - 1;
    }
    const long long nd = det_off[lo + 1] - det_off[lo], ng = gt_off[lo + 1] - gt_off[lo];
    if (nd <= 0 || nd > HF_KITTI_MAX_DET || ng > HF_KITTI_MAX_GT) return;
    const long long local = p - pair_off[lo], g = local / nd, d = local % nd;
    if (g >= ng) return;
    const double *a = det + (det_off[lo] + d) * kCols;        // detection (box a of the reference's overlap functions)
    const double *b = gt + (gt_off[lo] + g) * kCols;
    double *out = ov + p * 6;

    // imageBoxOverlap
    {
        const double x1 = smax(a[C_X1], b[C_X1]), y1 = smax(a[C_Y1], b[C_Y1]);
        const double x2 = smin(a[C_X2], b[C_X2]), y2 = smin(a[C_Y2], b[C_Y2]);
        const double w = x2 - x1, h = y2 - y1;
        if (w <= 0 || h <= 0) {
            out[0] = 0.0; out[3] = 0.0;
        } else {
            const double inter = w * h;
            const double a_area = (a[C_X2] - a[C_X1]) * (a[C_Y2] - a[C_Y1]);
            const double b_area = (b[C_X2] - b[C_X1]) * (b[C_Y2] - b[C_Y1]);
            out[0] = inter / (a_area + b_area - inter);
            out[3] = inter / a_area;
        }
    }
    // groundBoxOverlap / box3DOverlap: union = area(a) + area(b) - intersection
    double ax[4], az[4], bx[4], bz[4];
    bev_quad(a, ax, az);
    bev_quad(b, bx, bz);
    const double aa2 = area2(ax, az, 4), ba2 = area2(bx, bz, 4);
    const double inter = quad_intersection(ax, az, aa2, bx, bz, ba2);
    const double a_area = fabs(aa2) / 2, b_area = fabs(ba2) / 2;
    out[1] = inter / (a_area + b_area - inter);
    out[4] = inter / a_area;
    const double ymax = smin(a[C_T2], b[C_T2]);
    const double ymin = smax(a[C_T2] - a[C_H], b[C_T2] - b[C_H]);
    const double inter_vol = inter * smax(0.0, ymax - ymin);
    const double det_vol = a[C_H] * a[C_L] * a[C_W];
    const double gt_vol = b[C_H] * b[C_L] * b[C_W];
    out[2] = inter_vol / (det_vol + gt_vol - inter_vol);
    out[5] = inter_vol / det_vol;
}

// ------------------------------------------------------------------------------------------------ cleanData

// ignored_gt: 0 = counted, 1 = ignored (neighbour class, or filtered by the difficulty), -1 = other class
__device__ inline int gt_state(const double *r, int type, int occ, int cls, int diff)
{
    int valid;
    if (type == cls) valid = 1;
    else if ((cls == HF_KITTI_PEDESTRIAN && type == HF_KITTI_PERSON_SITTING) || (cls == HF_KITTI_CAR && type == HF_KITTI_VAN)) valid = 0;
    else valid = -1;
    const double height = r[C_Y2] - r[C_Y1];
    const bool ignore = occ > diff || r[C_EXTRA] > max_truncation(diff) || height <= (double)min_height(diff);
    if (valid == 1 && !ignore) return 0;
    if (valid == 0 || (ignore && valid == 1)) return 1;
    return -1;
}

// ignored_det: the height truncated to int32 (x86 cvttsd2si: NaN and out-of-range give INT_MIN) is tested first
__device__ inline int det_state(const double *r, int type, int cls, int diff)
{
    const double hf = fabs(r[C_Y1] - r[C_Y2]);
    const int height = (hf < 2147483648.0) ? (int)hf : INT_MIN;
    if (height < min_height(diff)) return 1;
    return type == cls ? 0 : -1;
}

struct Frame {
    long long g0, d0, p0;
    int ng, nd;
};

__device__ inline bool load_frame(int f, const long long *gt_off, const long long *det_off, const long long *pair_off, Frame &fr)
{
    fr.g0 = gt_off[f];
    fr.d0 = det_off[f];
    fr.p0 = pair_off[f];
    const long long ng = gt_off[f + 1] - fr.g0, nd = det_off[f + 1] - fr.d0;
    if (ng < 0 || nd < 0 || ng > HF_KITTI_MAX_GT || nd > HF_KITTI_MAX_DET) return false;
    fr.ng = (int)ng;
    fr.nd = (int)nd;
    return true;
}

// assigned-detection bits of one lane: mask[word * kThreads + lane] in LDS
struct Assigned {
    unsigned *m;
    __device__ void clear(int nd) { for (int w = 0; w < (nd + 31) / 32; ++w) m[w * kThreads] = 0u; }
    __device__ bool get(int j) const { return (m[(j >> 5) * kThreads] >> (j & 31)) & 1u; }
    __device__ void set(int j) { m[(j >> 5) * kThreads] |= 1u << (j & 31); }
};

// ------------------------------------------------------------------------------------------------ pass 1 (no FP)

__global__ void __launch_bounds__(kThreads) k_pass1(int frames, const long long *gt_off, const long long *det_off,
                                                    const long long *pair_off, long long n_gt, const double *gt,
                                                    const int *gt_type, const int *gt_occ, const double *det,
                                                    const int *det_type, const double *ov, const double *min_overlap,
                                                    int eval_mask, double *scores, int *n_tp, int *n_valid_gt)
{
    __shared__ unsigned mask[kMaskWords * kThreads];
    const int list = blockIdx.y;
    const int f = blockIdx.x * kThreads + threadIdx.x;
    if (f >= frames) return;
    const int metric = list / 9, cls = (list / 3) % 3, diff = list % 3;
    Frame fr;
    const bool ok = load_frame(f, gt_off, det_off, pair_off, fr);
    double *slot = scores + (long long)list * n_gt + (ok ? fr.g0 : 0);
    int ntp = 0, nvalid = 0;
    if (ok && ((eval_mask >> (list / 3)) & 1)) {
        const double minov = min_overlap[metric * 3 + cls];
        Assigned as{ mask + threadIdx.x };
        as.clear(fr.nd);
        for (int g = 0; g < fr.ng; ++g) {
            const double *gr = gt + (fr.g0 + g) * kCols;
            const int ig = gt_state(gr, gt_type[fr.g0 + g], gt_occ[fr.g0 + g], cls, diff);
            if (ig == 0) ++nvalid;
            if (ig == -1) continue;
            int det_idx = -1;
            double valid = kNoDetection;
            for (int j = 0; j < fr.nd; ++j) {
                const double *dr = det + (fr.d0 + j) * kCols;
                if (det_state(dr, det_type[fr.d0 + j], cls, diff) == -1) continue;
                if (as.get(j)) continue;
                const double o = ov[(fr.p0 + (long long)g * fr.nd + j) * 6 + metric];
                if (o > minov && dr[C_EXTRA] > valid) { det_idx = j; valid = dr[C_EXTRA]; }
            }
            if (valid == kNoDetection) continue;
            const double *dr = det + (fr.d0 + det_idx) * kCols;
            if (ig == 1 || det_state(dr, det_type[fr.d0 + det_idx], cls, diff) == 1) {
                as.set(det_idx);
            } else {
                slot[ntp++] = dr[C_EXTRA];
                as.set(det_idx);
            }
        }
    }
    if (ok)
        for (int k = ntp; k < fr.ng; ++k) slot[k] = -INFINITY;
    n_tp[list * frames + f] = ntp;
    n_valid_gt[list * frames + f] = nvalid;
}

// ------------------------------------------------------------------------------------------------ sort (descending, stable)

__global__ void __launch_bounds__(kThreads) k_merge(long long n, long long width, const double *src, double *dst)
{
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (long long)kLists * n) return;
    const long long base = (e / n) * n, i = e % n;
    const long long s = (i / (2 * width)) * (2 * width);
    const long long mid = s + width < n ? s + width : n, end = s + 2 * width < n ? s + 2 * width : n;
    const double x = src[base + i];
    long long out;
    if (i < mid) {                          // left element: after the right run's elements strictly greater than x
        long long lo = mid, hi = end;
        while (lo < hi) {
            const long long m = (lo + hi) >> 1;
            if (src[base + m] > x) lo = m + 1; else hi = m;
        }
        out = s + (i - s) + (lo - mid);
    } else {                                // right element: after the left run's elements greater than or equal to x
        long long lo = s, hi = mid;
        while (lo < hi) {
            const long long m = (lo + hi) >> 1;
            if (src[base + m] >= x) lo = m + 1; else hi = m;
        }
        out = s + (i - mid) + (lo - s);
    }
    dst[base + out] = x;
}

// ------------------------------------------------------------------------------------------------ thresholds

// getThresholds walks the sorted scores with current_recall += 1/40 after every selected rank; whether rank i is skipped,
// (r_recall - current) < (current - l_recall) with l = (i+1)/n_gt, r = (i+2)/n_gt, is monotone in i for a fixed current
// recall (every rounded operation is monotone), true up to some rank and false after it.  So the next selected rank is the
// first rank after the previous one that is not skipped: a binary search per recall step instead of a walk over every score.
__device__ inline bool skipped(long long i, double ngt, double current)
{
    const double l = (double)(i + 1) / ngt, r = (double)(i + 2) / ngt;
    return (r - current) < (current - l);
}

__global__ void __launch_bounds__(kThreads) k_thresholds(int frames, const int *n_tp, const int *n_valid_gt, const double *sorted,
                                                         long long n_gt, int eval_mask, double *thresholds, int *n_thresholds)
{
    __shared__ long long red[2][kThreads];
    const int list = blockIdx.x;
    long long a = 0, b = 0;
    for (int f = threadIdx.x; f < frames; f += kThreads) {
        a += n_tp[list * frames + f];
        b += n_valid_gt[list * frames + f];
    }
    red[0][threadIdx.x] = a;
    red[1][threadIdx.x] = b;
    __syncthreads();
    for (int s = kThreads / 2; s > 0; s >>= 1) {
        if (threadIdx.x < s) {
            red[0][threadIdx.x] += red[0][threadIdx.x + s];
            red[1][threadIdx.x] += red[1][threadIdx.x + s];
        }
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    double *thr = thresholds + list * kSteps;
    for (int t = 0; t < kSteps; ++t) thr[t] = 0.0;
    const long long nv = ((eval_mask >> (list / 3)) & 1) ? red[0][0] : 0;
    const double ngt = (double)red[1][0];
    const double *v = sorted + (long long)list * n_gt;
    double current = 0.0;
    int nt = 0;
    long long i = 0;
    while (i < nv && nt < kSteps) {
        long long lo = i, hi = nv - 1;      // first rank in [i, nv-1) that is not skipped, else the last rank
        while (lo < hi) {
            const long long m = (lo + hi) >> 1;
            if (skipped(m, ngt, current)) lo = m + 1; else hi = m;
        }
        thr[nt++] = v[lo];
        current += 1.0 / (kSteps - 1.0);
        i = lo + 1;
    }
    n_thresholds[list] = nt;
}

// ------------------------------------------------------------------------------------------------ pass 2 (per threshold)

__global__ void __launch_bounds__(kThreads) k_pass2(int frames, const long long *gt_off, const long long *det_off,
                                                    const long long *pair_off, const double *gt, const int *gt_type,
                                                    const int *gt_occ, const double *det, const int *det_type, const double *ov,
                                                    const double *min_overlap, int eval_mask, int compute_aos,
                                                    const double *thresholds, const int *n_thresholds, int *part_cnt,
                                                    double *part_sim)
{
    __shared__ unsigned mask[kMaskWords * kThreads];
    const int f = blockIdx.x;
    Frame fr;
    if (!load_frame(f, gt_off, det_off, pair_off, fr)) return;
    Assigned as{ mask + threadIdx.x };
    for (int task = threadIdx.x; task < kTasks; task += kThreads) {
        const int list = task / kSteps, t = task % kSteps;
        if (!((eval_mask >> (list / 3)) & 1) || t >= n_thresholds[list]) continue;
        const int metric = list / 9, cls = (list / 3) % 3, diff = list % 3;
        const double minov = min_overlap[metric * 3 + cls], thr = thresholds[list * kSteps + t];
        const bool sim_on = metric > 0 || compute_aos;
        as.clear(fr.nd);
        int tp = 0, fp = 0, fn = 0;
        double sim = 0.0;
        for (int g = 0; g < fr.ng; ++g) {
            const double *gr = gt + (fr.g0 + g) * kCols;
            const int ig = gt_state(gr, gt_type[fr.g0 + g], gt_occ[fr.g0 + g], cls, diff);
            if (ig == -1) continue;
            int det_idx = -1;
            double valid = kNoDetection, max_overlap = 0.0;
            bool assigned_ignored = false;
            for (int j = 0; j < fr.nd; ++j) {
                const double *dr = det + (fr.d0 + j) * kCols;
                const int id = det_state(dr, det_type[fr.d0 + j], cls, diff);
                if (id == -1 || as.get(j) || dr[C_EXTRA] < thr) continue;
                const double o = ov[(fr.p0 + (long long)g * fr.nd + j) * 6 + metric];
                if (o > minov && (o > max_overlap || assigned_ignored) && id == 0) {
                    max_overlap = o; det_idx = j; valid = 1; assigned_ignored = false;
                } else if (o > minov && valid == kNoDetection && id == 1) {
                    det_idx = j; valid = 1; assigned_ignored = true;
                }
            }
            if (valid == kNoDetection) {
                if (ig == 0) ++fn;
                continue;
            }
            const double *dr = det + (fr.d0 + det_idx) * kCols;
            if (ig == 1 || det_state(dr, det_type[fr.d0 + det_idx], cls, diff) == 1) {
                as.set(det_idx);
                continue;
            }
            ++tp;
            if (sim_on) {
                const double delta = metric == 0 ? gr[C_ALPHA] - dr[C_ALPHA] : fabs(gr[C_RY] - dr[C_RY]);
                sim += (1.0 + cos(delta)) / 2.0;
            }
            as.set(det_idx);
        }
        for (int j = 0; j < fr.nd; ++j) {
            const double *dr = det + (fr.d0 + j) * kCols;
            if (!(as.get(j) || det_state(dr, det_type[fr.d0 + j], cls, diff) != 0 || dr[C_EXTRA] < thr)) ++fp;
        }
        int nstuff = 0;                                   // DontCare rows, in GT order, absorb unassigned detections
        for (int g = 0; g < fr.ng; ++g) {
            if (gt_type[fr.g0 + g] != HF_KITTI_DONTCARE) continue;
            for (int j = 0; j < fr.nd; ++j) {
                const double *dr = det + (fr.d0 + j) * kCols;
                if (as.get(j) || det_state(dr, det_type[fr.d0 + j], cls, diff) != 0 || dr[C_EXTRA] < thr) continue;
                if (ov[(fr.p0 + (long long)g * fr.nd + j) * 6 + 3 + metric] > minov) {
                    as.set(j);
                    ++nstuff;
                }
            }
        }
        fp -= nstuff;
        const long long o = (long long)f * kTasks + task;
        part_cnt[o * 3 + 0] = tp;
        part_cnt[o * 3 + 1] = fp;
        part_cnt[o * 3 + 2] = fn;
        part_sim[o] = (tp > 0 || fp > 0) ? sim : -1.0;
    }
}

// ------------------------------------------------------------------------------------------------ finalize

constexpr int kChunk = 16;

__global__ void __launch_bounds__(64) k_finalize(int frames, int eval_mask, int compute_aos, const int *n_thresholds,
                                                 const int *part_cnt, const double *part_sim, int *counts, double *precision,
                                                 double *aos, double *aos_ground)
{
    __shared__ double pr[kSteps], sm[kSteps];
    const int list = blockIdx.x, t = threadIdx.x, metric = list / 9;
    const int nt = ((eval_mask >> (list / 3)) & 1) ? n_thresholds[list] : 0;
    const bool sim_on = metric > 0 || compute_aos;
    if (t < kSteps) {
        long long tp = 0, fp = 0, fn = 0;
        double sim = 0.0;
        if (t < nt) {
            const int task = list * kSteps + t;
            for (int f0 = 0; f0 < frames; f0 += kChunk) {   // loads of a chunk issued together, added in frame order
                const int n = frames - f0 < kChunk ? frames - f0 : kChunk;
                double s[kChunk];
                int c[kChunk][3];
#pragma unroll
                for (int k = 0; k < kChunk; ++k)
                    if (k < n) {
                        const long long o = (long long)(f0 + k) * kTasks + task;
                        s[k] = part_sim[o];
                        c[k][0] = part_cnt[o * 3];
                        c[k][1] = part_cnt[o * 3 + 1];
                        c[k][2] = part_cnt[o * 3 + 2];
                    }
#pragma unroll
                for (int k = 0; k < kChunk; ++k)
                    if (k < n) {
                        tp += c[k][0];
                        fp += c[k][1];
                        fn += c[k][2];
                        if (s[k] != -1.0) sim += s[k];
                    }
            }
        }
        int *cnt = counts + (list * kSteps + t) * 3;
        cnt[0] = (int)tp;
        cnt[1] = (int)fp;
        cnt[2] = (int)fn;
        pr[t] = t < nt ? tp / (double)(tp + fp) : 0.0;
        sm[t] = t < nt && sim_on ? sim / (double)(tp + fp) : 0.0;
    }
    __syncthreads();
    if (t >= kSteps) return;
    double p = pr[t], a = sm[t];
    if (t < nt) {                                         // *max_element(begin + t, end): the first largest by operator<
        int lp = t, la = t;
        for (int k = t + 1; k < kSteps; ++k) {
            if (pr[lp] < pr[k]) lp = k;
            if (sm[la] < sm[k]) la = k;
        }
        p = pr[lp];
        a = sm[la];
    }
    precision[list * kSteps + t] = p;
    aos[list * kSteps + t] = metric == 0 ? a : 0.0;
    aos_ground[list * kSteps + t] = metric > 0 ? a : 0.0;
}

inline size_t pad256(size_t b) { return (b + 255) & ~size_t(255); }

struct Layout {
    size_t ov, sa, sb, ntp, nvalid, cnt, sim, total;
};

Layout layout(int frames, long long n_gt, long long n_pairs)
{
    Layout l;
    size_t o = 0;
    l.ov = o;     o += pad256((size_t)n_pairs * 6 * sizeof(double));
    l.sa = o;     o += pad256((size_t)kLists * n_gt * sizeof(double));
    l.sb = o;     o += pad256((size_t)kLists * n_gt * sizeof(double));
    l.ntp = o;    o += pad256((size_t)kLists * frames * sizeof(int));
    l.nvalid = o; o += pad256((size_t)kLists * frames * sizeof(int));
    l.cnt = o;    o += pad256((size_t)frames * kTasks * 3 * sizeof(int));
    l.sim = o;    o += pad256((size_t)frames * kTasks * sizeof(double));
    l.total = o;
    return l;
}

bool sizes_ok(int frames, long long n_gt, long long n_det, long long n_pairs, int max_gt, int max_det)
{
    return frames > 0 && frames <= (1 << 24) && max_gt >= 0 && max_gt <= HF_KITTI_MAX_GT && max_det >= 0 &&
           max_det <= HF_KITTI_MAX_DET && n_gt >= 0 && n_det >= 0 && n_pairs >= 0 && n_gt <= (long long)frames * max_gt &&
           n_det <= (long long)frames * max_det && n_pairs <= (long long)frames * max_gt * max_det;
}

int launch_overlaps(int frames, const long long *gt_off, const long long *det_off, const long long *pair_off, long long n_pairs,
                    const double *gt, const double *det, double *ov, hipStream_t st)
{
    if (n_pairs == 0) return HF_OK;
    hipLaunchKernelGGL(k_overlaps, dim3(div_up(n_pairs, kThreads)), dim3(kThreads), 0, st, frames, gt_off, det_off, pair_off,
                       n_pairs, gt, det, ov);
    return launch_status();
}

}  // namespace

}  // namespace hf

using namespace hf;

HF_API size_t hf_kitti_eval_workspace(int n_frames, long long n_gt, long long n_pairs)
{
    if (n_frames <= 0 || n_gt < 0 || n_pairs < 0) return 0;
    return layout(n_frames, n_gt, n_pairs).total;
}

HF_API int hf_kitti_eval_overlaps(int n_frames, const long long *gt_off, const long long *det_off, const long long *pair_off,
                                  long long n_gt, long long n_det, long long n_pairs, int max_gt, int max_det, const double *gt,
                                  const double *det, double *overlaps, hf_stream_t stream)
{
    if (!sizes_ok(n_frames, n_gt, n_det, n_pairs, max_gt, max_det)) return HF_EINVAL;
    if (!gt_off || !det_off || !pair_off) return HF_EINVAL;
    if (n_pairs > 0 && (!gt || !det || !overlaps)) return HF_EINVAL;
    return launch_overlaps(n_frames, gt_off, det_off, pair_off, n_pairs, gt, det, overlaps, as_stream(stream));
}

HF_API int hf_kitti_eval(int n_frames, const long long *gt_off, const long long *det_off, const long long *pair_off, long long n_gt,
                         long long n_det, long long n_pairs, int max_gt, int max_det, const double *gt, const int *gt_type,
                         const int *gt_occ, const double *det, const int *det_type, const double *min_overlap, int eval_mask,
                         int compute_aos, double *thresholds, int *n_thresholds, int *counts, double *precision, double *aos,
                         double *aos_ground, void *workspace, size_t workspace_bytes, hf_stream_t stream)
{
    if (!sizes_ok(n_frames, n_gt, n_det, n_pairs, max_gt, max_det) || eval_mask < 0 || eval_mask > 511) return HF_EINVAL;
    if (!gt_off || !det_off || !pair_off || !min_overlap || !thresholds || !n_thresholds || !counts || !precision || !aos ||
        !aos_ground)
        return HF_EINVAL;
    if ((n_gt > 0 && (!gt || !gt_type || !gt_occ)) || (n_det > 0 && (!det || !det_type))) return HF_EINVAL;
    const Layout l = layout(n_frames, n_gt, n_pairs);
    if (!workspace || workspace_bytes < l.total) return HF_EWORKSPACE;
    hipStream_t st = as_stream(stream);
    char *ws = static_cast<char *>(workspace);
    double *ov = reinterpret_cast<double *>(ws + l.ov);
    double *sa = reinterpret_cast<double *>(ws + l.sa), *sb = reinterpret_cast<double *>(ws + l.sb);
    int *ntp = reinterpret_cast<int *>(ws + l.ntp), *nvalid = reinterpret_cast<int *>(ws + l.nvalid);
    int *pcnt = reinterpret_cast<int *>(ws + l.cnt);
    double *psim = reinterpret_cast<double *>(ws + l.sim);

    int s = launch_overlaps(n_frames, gt_off, det_off, pair_off, n_pairs, gt, det, ov, st);
    if (s != HF_OK) return s;
    hipLaunchKernelGGL(k_pass1, dim3(div_up(n_frames, kThreads), kLists), dim3(kThreads), 0, st, n_frames, gt_off, det_off, pair_off,
                       n_gt, gt, gt_type, gt_occ, det, det_type, ov, min_overlap, eval_mask, sa, ntp, nvalid);
    if ((s = launch_status()) != HF_OK) return s;
    double *src = sa, *dst = sb;
    for (long long w = 1; w < n_gt; w *= 2) {
        hipLaunchKernelGGL(k_merge, dim3(div_up(kLists * n_gt, kThreads)), dim3(kThreads), 0, st, n_gt, w, src, dst);
        if ((s = launch_status()) != HF_OK) return s;
        double *tmp = src; src = dst; dst = tmp;
    }
    hipLaunchKernelGGL(k_thresholds, dim3(kLists), dim3(kThreads), 0, st, n_frames, ntp, nvalid, src, n_gt, eval_mask, thresholds,
                       n_thresholds);
    if ((s = launch_status()) != HF_OK) return s;
    hipLaunchKernelGGL(k_pass2, dim3(n_frames), dim3(kThreads), 0, st, n_frames, gt_off, det_off, pair_off, gt, gt_type, gt_occ, det,
                       det_type, ov, min_overlap, eval_mask, compute_aos, thresholds, n_thresholds, pcnt, psim);
    if ((s = launch_status()) != HF_OK) return s;
    hipLaunchKernelGGL(k_finalize, dim3(kLists), dim3(64), 0, st, n_frames, eval_mask, compute_aos, n_thresholds, pcnt, psim, counts,
                       precision, aos, aos_ground);
    return launch_status();
}
