// rcnn_targets.hip -- the RCNN's proposal-target layer on the device (hf/datasets/kitti/kitti_dataset.py:509-513 val
// assignment, :545-680 sample_rois_for_rcnn_training / sample_bg_inds, :690-770 aug_roi_by_noise / random_aug_box3d).
// The reference runs it in the host data loader (a NumPy loop calling shapely per RoI); here it is three launches that a
// captured train step replays:
//   iou     one thread per (frame, proposal, gt) pair: the 3D IoU of hf/core/compute_iou.py:23-64 (modules.box3d_iou) --
//           the BEV overlap of bev_iou.hip evaluated by one thread (same helpers, same order of operations, same bits),
//           then the height overlap and volumes in the order the torch form writes them.  Block 0 also snapshots the RNG
//           state into the workspace and advances the call counter (rng_state[1]) for the next call;
//   sample  one workgroup per frame: per-RoI max / first argmax over the GTs, per-GT argmax RoI, the fg / easy bg / hard bg
//           lists in ascending order (one thread: m + g steps), the branch, the random permutation of the fg list (partial
//           Fisher-Yates, one thread, <= R steps), then one thread per output slot;
//   jitter  one thread per sampled RoI (fg: up to 10 tries, bg: 1 try), the IoU against its ASSIGNED gt.
// Random numbers are a counter hash of (base seed, call number, frame, slot, draw); they do not follow NumPy's stream.
// Pinned by tests/test_sampler_abi.py against the NumPy restatement of tests/sampler_cases.py: every draw (the hash is pure
// integer arithmetic), every rule and branch, rois under 'single' / 'multiple' bit for bit, the 3D IoU against an fp64 clip.
#include <math.h>

#include "bev_common.h"
#include "box3d_common.h"
#include "hf_common.h"

namespace hf {

constexpr int kTgtMaxB = 1024, kTgtMaxM = 512, kTgtMaxG = 128, kTgtMaxR = 512, kTgtThreads = 256;
constexpr int kTgtFgTries = 10, kTgtBgTries = 1;

// box_overlap_serial and box3d_iou_dev (the one-thread clip and the 3D IoU of one pair) live in box3d_common.h, shared with
// eval_stats.hip.

// ---------------------------------------------------------------- random numbers
__device__ __forceinline__ unsigned long long splitmix64(unsigned long long z)
{
    z += 0x9e3779b97f4a7c15ull;
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

// the key of one call: (base seed, call number) as the workspace snapshot holds them
__device__ __forceinline__ unsigned long long tgt_key(const unsigned long long *snap)
{
    return splitmix64(snap[0] + snap[1] * 0xd1b54a32d192ed03ull);
}

// uniform in [0, 1) (24 bits) of draw `draw` of slot `slot` of frame `frame`
__device__ __forceinline__ float tgt_uniform(unsigned long long key, int frame, int slot, int draw)
{
    const unsigned long long ctr = (static_cast<unsigned long long>(frame) << 40) | (static_cast<unsigned long long>(slot) << 16) |
                                   static_cast<unsigned long long>(draw);
    return static_cast<float>(splitmix64(key ^ splitmix64(ctr)) >> 40) * (1.0f / 16777216.0f);
}

// floor(u * size) as the reference's index draws, kept below size (u * size can round up to size in fp32)
__device__ __forceinline__ int tgt_index(float u, int size)
{
    const int i = static_cast<int>(floorf(u * static_cast<float>(size)));
    return i < size - 1 ? i : size - 1;
}

// draw numbers: 0 the fg permutation step, 1 the with-replacement index of a slot, 16 + 16 t + c the jitter try t
constexpr int kDrawPerm = 0, kDrawIndex = 1, kDrawJitter = 16;

// ---------------------------------------------------------------- workspace
__host__ __device__ inline size_t tgt_align(size_t v) { return (v + 255) & ~static_cast<size_t>(255); }
__host__ __device__ inline size_t tgt_ws_tries_offset(int b, int m, int g) { return tgt_align(sizeof(float) * static_cast<size_t>(b) * m * g); }
__host__ __device__ inline size_t tgt_ws_rng_offset(int b, int m, int g) { return tgt_ws_tries_offset(b, m, g) + tgt_align(sizeof(int) * static_cast<size_t>(b) * kTgtMaxR); }
__host__ __device__ inline size_t tgt_ws_bytes(int b, int m, int g) { return tgt_ws_rng_offset(b, m, g) + 256; }

struct TgtArgs {
    int b, m, g, r;
    const float *proposals;       // (b, m, 7)
    const int *pcount, *gcount;   // (b)
    const float *gt;              // (b, g, 8)
    float neg_lo, neg_hi, fg_thresh, hard_ratio;
    int fg_per_image, aug, train;
    const float *iou;             // workspace (b, m, g)
    int *tries;                   // workspace (b, kTgtMaxR)
    unsigned long long *snap;     // workspace: base seed, call number of this call
    float *rois, *iou_out, *gt_out;
    int *stats;
};

__global__ __launch_bounds__(256) void rcnn_iou_kernel(TgtArgs a, long long *__restrict__ rng_state, float *__restrict__ iou)
{
    const long long idx = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (idx == 0 && rng_state) {
        a.snap[0] = static_cast<unsigned long long>(rng_state[0]);
        a.snap[1] = static_cast<unsigned long long>(rng_state[1]);
        rng_state[1] = rng_state[1] + 1;   // the next call (the next replay) draws fresh samples
    }
    const long long total = static_cast<long long>(a.b) * a.m * a.g;
    if (idx >= total) return;
    const int j = static_cast<int>(idx % a.g);
    const int i = static_cast<int>((idx / a.g) % a.m);
    const int f = static_cast<int>(idx / (static_cast<long long>(a.g) * a.m));
    if (i >= a.pcount[f] || j >= a.gcount[f]) return;   // padding: never read
    iou[idx] = box3d_iou_dev(a.proposals + (static_cast<long long>(f) * a.m + i) * 7, a.gt + (static_cast<long long>(f) * a.g + j) * 8);
}

__device__ __forceinline__ void tgt_write(const TgtArgs &a, int f, int s, int roi, int ng, const float *s_max, const int *s_arg)
{
    const long long o = static_cast<long long>(f) * a.r + s;
    float *ro = a.rois + o * 7, *go = a.gt_out + o * 8;
    if (roi < 0) {   // no proposal in this frame
        for (int d = 0; d < 7; ++d) ro[d] = 0.0f;
        for (int d = 0; d < 8; ++d) go[d] = 0.0f;
        a.iou_out[o] = 0.0f;
        return;
    }
    const float *src = a.proposals + (static_cast<long long>(f) * a.m + roi) * 7;
    for (int d = 0; d < 7; ++d) ro[d] = src[d];
    if (ng > 0) {
        const float *gs = a.gt + (static_cast<long long>(f) * a.g + s_arg[roi]) * 8;
        for (int d = 0; d < 8; ++d) go[d] = gs[d];
    } else {
        for (int d = 0; d < 8; ++d) go[d] = 0.0f;
    }
    a.iou_out[o] = s_max[roi];
}

__global__ __launch_bounds__(kTgtThreads) void rcnn_sample_kernel(TgtArgs a)
{
    __shared__ float s_max[kTgtMaxM];
    __shared__ int s_arg[kTgtMaxM];
    __shared__ float g_max[kTgtMaxG];
    __shared__ int g_arg[kTgtMaxG];
    __shared__ int s_fg[kTgtMaxM + kTgtMaxG], s_easy[kTgtMaxM], s_hard[kTgtMaxM];
    __shared__ int s_cnt[5];   // #fg, #easy, #hard, fg slots, bg slots
    const int f = blockIdx.x, t = threadIdx.x;
    const int n = min(max(a.pcount[f], 0), a.m), ng = min(max(a.gcount[f], 0), a.g);
    const float *iou = a.iou + static_cast<long long>(f) * a.m * a.g;
    // ---- per RoI: max and first argmax over the GTs (a frame without GT: IoU 0, every RoI easy bg)
    for (int i = t; i < n; i += kTgtThreads) {
        float mx = 0.0f;
        int am = 0;
        if (ng > 0) {
            mx = iou[i * a.g];
            for (int j = 1; j < ng; ++j) {
                const float v = iou[i * a.g + j];
                if (v > mx) { mx = v; am = j; }
            }
        }
        s_max[i] = mx;
        s_arg[i] = am;
    }
    // ---- per GT: max and first argmax over the RoIs
    for (int j = t; j < ng; j += kTgtThreads) {
        float mx = n > 0 ? iou[j] : 0.0f;
        int am = 0;
        for (int i = 1; i < n; ++i) {
            const float v = iou[i * a.g + j];
            if (v > mx) { mx = v; am = i; }
        }
        g_max[j] = mx;
        g_arg[j] = am;
    }
    __syncthreads();
    if (!a.train) {   // val (:509-513): every proposal with its max IoU and argmax GT, no sampling (r == m)
        for (int s = t; s < a.r; s += kTgtThreads) tgt_write(a, f, s, s < n ? s : -1, ng, s_max, s_arg);
    }
    unsigned long long key = 0;
    if (a.train) key = tgt_key(a.snap);
    if (t == 0) {
        int nfg = 0, ne = 0, nh = 0;
        for (int i = 0; i < n; ++i)
            if (s_max[i] >= a.fg_thresh) s_fg[nfg++] = i;
        for (int j = 0; j < ng; ++j)
            if (g_max[j] > 0.0f) s_fg[nfg++] = g_arg[j];   // the RoI that overlaps a GT most is fg too (duplicates kept)
        for (int i = 0; i < n; ++i) {
            if (s_max[i] < a.neg_lo) s_easy[ne++] = i;
            else if (s_max[i] < a.neg_hi) s_hard[nh++] = i;
        }
        int fg_slots = 0, bg_slots = 0;
        if (a.train) {
            if (nfg > 0 && ne + nh > 0) {
                fg_slots = min(a.fg_per_image, nfg);
                for (int s = 0; s < fg_slots; ++s) {   // the first fg_slots entries of a random permutation
                    const int j = s + tgt_index(tgt_uniform(key, f, s, kDrawPerm), nfg - s);
                    const int tmp = s_fg[s]; s_fg[s] = s_fg[j]; s_fg[j] = tmp;
                }
                bg_slots = a.r - fg_slots;
            } else if (nfg > 0) {
                fg_slots = a.r;
            } else if (ne + nh > 0) {
                bg_slots = a.r;
            }
        }
        s_cnt[0] = nfg; s_cnt[1] = ne; s_cnt[2] = nh; s_cnt[3] = fg_slots; s_cnt[4] = bg_slots;
        if (a.stats) {
            int *st = a.stats + 4 * f;
            st[0] = nfg; st[1] = ne + nh; st[2] = fg_slots; st[3] = bg_slots;
        }
    }
    if (!a.train) return;
    __syncthreads();
    const int nfg = s_cnt[0], ne = s_cnt[1], nh = s_cnt[2], fg_slots = s_cnt[3], bg_slots = s_cnt[4];
    const int hard_slots = (nh > 0 && ne > 0) ? static_cast<int>(static_cast<float>(bg_slots) * a.hard_ratio) : (nh > 0 ? bg_slots : 0);
    for (int s = t; s < a.r; s += kTgtThreads) {
        int roi, tries;
        if (n == 0) {
            roi = -1; tries = 0;
        } else if (s < fg_slots) {
            roi = (nfg > 0 && ne + nh > 0) ? s_fg[s] : s_fg[tgt_index(tgt_uniform(key, f, s, kDrawIndex), nfg)];
            tries = kTgtFgTries;
        } else if (bg_slots > 0) {
            const int q = s - fg_slots;   // hard bg first, then easy (sample_bg_inds)
            const float u = tgt_uniform(key, f, s, kDrawIndex);
            roi = q < hard_slots ? s_hard[tgt_index(u, nh)] : s_easy[tgt_index(u, ne)];
            tries = kTgtBgTries;
        } else {
            // neither fg nor bg (the reference stops in pdb): any RoI of the frame, with replacement, no jitter
            roi = tgt_index(tgt_uniform(key, f, s, kDrawIndex), n);
            tries = 0;
        }
        if (a.aug == 0 || ng == 0) tries = 0;
        a.tries[static_cast<long long>(f) * kTgtMaxR + s] = tries;
        tgt_write(a, f, s, roi, ng, s_max, s_arg);
    }
}

// random_aug_box3d (:722-770) for one try
__device__ void random_aug_box3d(int method, unsigned long long key, int f, int s, int base, const float *in, float *out)
{
    auto u = [&](int c) { return tgt_uniform(key, f, s, base + c); };
    if (method == 1) {            // 'single'
        for (int d = 0; d < 3; ++d) out[d] = in[d] + (u(1 + d) - 0.5f);
        for (int d = 0; d < 3; ++d) out[3 + d] = in[3 + d] * ((u(4 + d) - 0.5f) / (0.5f / 0.15f) + 1.0f);
        out[6] = in[6] + (u(7) - 0.5f) / (0.5f / (static_cast<float>(M_PI) / 12.0f));
    } else if (method == 2) {     // 'multiple': pos_range, hwl_range, angle_range of the five rows
        const float pos_r[5] = { 0.2f, 0.3f, 0.5f, 0.8f, 1.0f };
        const float hwl_r[5] = { 0.1f, 0.15f, 0.15f, 0.15f, 0.15f };
        const float ang_r[5] = { static_cast<float>(M_PI / 12), static_cast<float>(M_PI / 12), static_cast<float>(M_PI / 9),
                                 static_cast<float>(M_PI / 6), static_cast<float>(M_PI / 3) };
        const int row = tgt_index(u(1), 5);
        for (int d = 0; d < 3; ++d) out[d] = in[d] + ((u(2 + d) - 0.5f) / 0.5f) * pos_r[row];
        for (int d = 0; d < 3; ++d) out[3 + d] = in[3 + d] * (((u(5 + d) - 0.5f) / 0.5f) * hwl_r[row] + 1.0f);
        out[6] = in[6] + ((u(8) - 0.5f) / 0.5f) * ang_r[row];
    } else {                      // 'normal': x, y, z, [3], [4], [5] shifted by N(0, sigma), ry uniform in +-pi/12
        const float sigma[6] = { 0.3f, 0.2f, 0.3f, 0.25f, 0.15f, 0.5f };
        for (int d = 0; d < 6; ++d) {
            const float u1 = 1.0f - u(1 + 2 * d), u2 = u(2 + 2 * d);   // Box-Muller, u1 in (0, 1]
            out[d] = in[d] + sigma[d] * sqrtf(-2.0f * logf(u1)) * cosf(2.0f * static_cast<float>(M_PI) * u2);
        }
        out[6] = in[6] + ((u(13) - 0.5f) / 0.5f) * static_cast<float>(M_PI) / 12.0f;
    }
}

// aug_roi_by_noise (:690-720): keep the RoI with probability 0.2, else a random box; stop at IoU >= fg_thresh with the
// assigned GT or after the slot's tries; the IoU of the last box is the slot's IoU
__global__ __launch_bounds__(256) void rcnn_jitter_kernel(TgtArgs a)
{
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= a.b * a.r) return;
    const int f = idx / a.r, s = idx % a.r;
    const int tries = a.tries[static_cast<long long>(f) * kTgtMaxR + s];
    if (tries == 0) return;
    const unsigned long long key = tgt_key(a.snap);
    float *ro = a.rois + static_cast<long long>(idx) * 7;
    float roi[7], gtb[7], cur[7];
    for (int d = 0; d < 7; ++d) { roi[d] = ro[d]; cur[d] = ro[d]; gtb[d] = a.gt_out[static_cast<long long>(idx) * 8 + d]; }
    float tiou = 0.0f;
    for (int c = 0; tiou < a.fg_thresh && c < tries; ++c) {
        const int base = kDrawJitter + 16 * c;
        if (tgt_uniform(key, f, s, base) < 0.2f) {
            for (int d = 0; d < 7; ++d) cur[d] = roi[d];
        } else {
            random_aug_box3d(a.aug, key, f, s, base, roi, cur);
        }
        tiou = box3d_iou_dev(cur, gtb);
    }
    for (int d = 0; d < 7; ++d) ro[d] = cur[d];
    a.iou_out[idx] = tiou;
}

// the (b, m, g) 3D IoU matrix of hf_box3d_iou_matrix: the pairs of rcnn_iou_kernel through the same box3d_iou_dev, zeros in the
// padding (a proposal row >= proposal_count[f] or a GT column >= gt_count[f])
__global__ __launch_bounds__(256) void box3d_iou_matrix_kernel(int b, int m, int g, const float *__restrict__ proposals,
                                                               const int *__restrict__ pcount, const float *__restrict__ gt,
                                                               const int *__restrict__ gcount, float *__restrict__ iou)
{
    const long long idx = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
    const long long total = static_cast<long long>(b) * m * g;
    if (idx >= total) return;
    const int j = static_cast<int>(idx % g);
    const int i = static_cast<int>((idx / g) % m);
    const int f = static_cast<int>(idx / (static_cast<long long>(g) * m));
    float v = 0.0f;
    if (i < pcount[f] && j < gcount[f])
        v = box3d_iou_dev(proposals + (static_cast<long long>(f) * m + i) * 7, gt + (static_cast<long long>(f) * g + j) * 8);
    iou[idx] = v;
}

}  // namespace hf

using namespace hf;

HF_API size_t hf_rcnn_targets_workspace(int b, int m, int g)
{
    if (b < 0 || b > kTgtMaxB || m < 1 || m > kTgtMaxM || g < 0 || g > kTgtMaxG) return 0;
    return tgt_ws_bytes(b, m, g);
}

HF_API int hf_rcnn_proposal_targets(int b, int m, int g, const float *proposals, const int *proposal_count, const float *gt,
                                    const int *gt_count, float cls_neg_lo, float cls_neg_hi, float cls_pos_lo, float reg_pos_lo,
                                    int roi_per_sample, float fg_ratio, float hard_bg_ratio, int aug_method, int train,
                                    long long *rng_state, float *rois, float *iou_of_rois, float *gt_of_rois, int *stats,
                                    void *workspace, size_t workspace_bytes, hf_stream_t stream)
{
    if (b < 0 || b > kTgtMaxB || m < 1 || m > kTgtMaxM || g < 0 || g > kTgtMaxG) return HF_EINVAL;
    if (roi_per_sample <= 0 || roi_per_sample > kTgtMaxR || aug_method < 0 || aug_method > 3) return HF_EINVAL;
    if (!(fg_ratio >= 0.0f && fg_ratio <= 1.0f) || !(hard_bg_ratio >= 0.0f && hard_bg_ratio <= 1.0f)) return HF_EINVAL;
    if (!(cls_neg_lo <= cls_neg_hi) || !(reg_pos_lo == reg_pos_lo) || !(cls_pos_lo == cls_pos_lo)) return HF_EINVAL;
    if (!train && roi_per_sample != m) return HF_EINVAL;   // val: one output row per proposal
    if (b == 0) return HF_OK;
    if (!proposals || !proposal_count || !gt_count || (g > 0 && !gt) || !rois || !iou_of_rois || !gt_of_rois) return HF_EINVAL;
    if (train && !rng_state) return HF_EINVAL;
    if (!workspace || workspace_bytes < tgt_ws_bytes(b, m, g)) return HF_EWORKSPACE;
    unsigned char *ws = static_cast<unsigned char *>(workspace);
    TgtArgs a;
    a.b = b; a.m = m; a.g = g; a.r = roi_per_sample;
    a.proposals = proposals; a.pcount = proposal_count; a.gcount = gt_count; a.gt = gt;
    a.neg_lo = cls_neg_lo; a.neg_hi = cls_neg_hi; a.fg_thresh = fminf(reg_pos_lo, cls_pos_lo); a.hard_ratio = hard_bg_ratio;
    a.fg_per_image = static_cast<int>(nearbyint(static_cast<double>(fg_ratio) * roi_per_sample));   // np.round: half to even
    a.aug = aug_method; a.train = train;
    a.iou = reinterpret_cast<const float *>(ws);
    a.tries = reinterpret_cast<int *>(ws + tgt_ws_tries_offset(b, m, g));
    a.snap = reinterpret_cast<unsigned long long *>(ws + tgt_ws_rng_offset(b, m, g));
    a.rois = rois; a.iou_out = iou_of_rois; a.gt_out = gt_of_rois; a.stats = stats;
    hipStream_t st = as_stream(stream);
    const long long pairs = static_cast<long long>(b) * m * g;
    hipLaunchKernelGGL(rcnn_iou_kernel, dim3(pairs > 0 ? div_up(pairs, 256) : 1), dim3(256), 0, st, a, train ? rng_state : nullptr,
                       reinterpret_cast<float *>(ws));
    hipLaunchKernelGGL(rcnn_sample_kernel, dim3(b), dim3(kTgtThreads), 0, st, a);
    if (train && aug_method != 0)
        hipLaunchKernelGGL(rcnn_jitter_kernel, dim3(div_up(static_cast<long long>(b) * roi_per_sample, 256)), dim3(256), 0, st, a);
    return launch_status();
}

HF_API int hf_box3d_iou_matrix(int b, int m, int g, const float *proposals, const int *proposal_count, const float *gt,
                               const int *gt_count, float *iou, hf_stream_t stream)
{
    if (b < 0 || b > kTgtMaxB || m < 1 || m > kTgtMaxM || g < 0 || g > kTgtMaxG) return HF_EINVAL;
    if (b == 0 || g == 0) return HF_OK;
    if (!proposals || !proposal_count || !gt || !gt_count || !iou) return HF_EINVAL;
    const long long pairs = static_cast<long long>(b) * m * g;
    hipLaunchKernelGGL(box3d_iou_matrix_kernel, dim3(div_up(pairs, 256)), dim3(256), 0, as_stream(stream), b, m, g, proposals,
                       proposal_count, gt, gt_count, iou);
    return launch_status();
}
