// rpn_batch.hip -- the RPN's training sample on the device (hf/datasets/kitti/kitti_dataset.py:291-440 load_rpn_samples and
// generate_rpn_training_labels, hf/datasets/kitti/kitti_aug.py).  The reference builds each sample on the host in NumPy; here
// a batch of B frames is three entry points that read the packed raw files (one host-to-device copy per buffer):
//   points   classify  one thread per raw point: fp64 velodyne -> rect transform, z > 0, strictly inside the ORIGINAL image
//                      under the original P2 (obj_utils.py:221-275); near (depth < 40 m) / far; per-block counts.  Block
//                      (0, 0) snapshots the RNG state and advances the call number;
//            scan      one workgroup per frame: exclusive scan of the block counts, n_near / n_far / n, the frame's status;
//            place     one thread per raw point: its near / far / kept rank in index order (wave ballots), selection without
//                      replacement by a keyed permutation of the rank, its output slot by a second permutation of [0, P);
//            fill      one thread per output slot: empty frames (zeros) and the with-replacement extra draws;
//   labels   one thread per sampled point, the frame's boxes in LDS: the reference's last-box-wins rule with the ring of
//            the enlarged box marked -1, corner form of obj_utils.is_point_inside (strict on every face), fp64;
//   image    sums      integer sums of x and x x^T per block (frames with PCA jitter only);
//            pca       one workgroup per frame: exact covariance, 3x3 Jacobi in fp64, the noise vector;
//            resize    one thread per output pixel: flip, jitter of the four source pixels, bilinear resize (cv2 INTER_LINEAR
//                      geometry, fp32 weights, rounded to nearest).
// Random numbers are a counter hash of (seed, call number, frame, purpose, index); they do not follow NumPy's stream.  Every
// output element has exactly one writer and no float is accumulated with atomics: a given rng_state gives the same bits.
// tests/test_sampler_abi.py holds every draw, slot and pixel to the NumPy restatement of tests/sampler_cases.py.
// The keyed permutation (4 Feistel rounds, round function masked to half the even bit count, cycle walk) is measurably
// non-uniform on tiny domains: over 20 000 keys a host prototype is 11 sigma off in single-element inclusion counts at
// n = 5 and has a position chi-square of 580 against 361 degrees of freedom at n = 20; from n = 64 up it is
// indistinguishable from uniform (4034 against 3969 at n = 64, 89 858 against 89 401 at n = 300).  The training path
// permutes thousands of points; changing the hash would change every seeded run and the exported hand-off files.
#include <math.h>

#include "hf_common.h"

namespace hf {

constexpr int kRbMaxB = 1024, kRbThreads = 256, kRbMaxG = 128, kRbMaxP = 1 << 20;
constexpr long long kRbMaxFrame = 1ll << 30;
constexpr int kRbImgPixPerThread = 16, kRbImgMaxSide = 8192;
constexpr long long kRbImgMaxPixels = 1ll << 23;   // N * sum(x x^T) stays exact in int64
constexpr double kRbFarDepth = 40.0;

// purposes of the counter hash
constexpr unsigned kRbNear = 1, kRbFar = 2, kRbExtra = 3, kRbDraw = 4, kRbShuffle = 5, kRbNormal = 6;

// ---------------------------------------------------------------- random numbers
__device__ __forceinline__ unsigned long long rb_mix(unsigned long long z)
{
    z += 0x9e3779b97f4a7c15ull;
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

// the key of (call, frame, purpose): snap = [base seed, call number] as the workspace holds them
__device__ __forceinline__ unsigned long long rb_key(const unsigned long long *snap, int frame, unsigned purpose)
{
    const unsigned long long call = rb_mix(snap[0] + snap[1] * 0xd1b54a32d192ed03ull);
    return rb_mix(call ^ ((static_cast<unsigned long long>(frame) << 8) | purpose));
}

// a keyed bijection of [0, n): a 4-round Feistel network on the next even power of two >= n, cycle-walked back into [0, n)
struct RbPerm {
    unsigned long long key;
    unsigned n, mask;
    int half;
};

__device__ __forceinline__ RbPerm rb_perm(unsigned long long key, unsigned n)
{
    int bits = 2;
    while ((1u << bits) < n) ++bits;
    bits += bits & 1;
    RbPerm p;
    p.key = key; p.n = n; p.half = bits / 2; p.mask = (1u << (bits / 2)) - 1u;
    return p;
}

__device__ __forceinline__ unsigned rb_apply(const RbPerm &p, unsigned x)
{
    do {
        unsigned l = x >> p.half, r = x & p.mask;
        for (unsigned round = 0; round < 4; ++round) {
            const unsigned f = static_cast<unsigned>(rb_mix(p.key ^ ((static_cast<unsigned long long>(round) << 32) | r))) & p.mask;
            const unsigned nl = r;
            r = l ^ f;
            l = nl;
        }
        x = (l << p.half) | r;
    } while (x >= p.n);   // x stays on the cycle of the original element, which returns into [0, n)
    return x;
}

// uniform index in [0, n) of draw `i` under `key`
__device__ __forceinline__ unsigned rb_index(unsigned long long key, unsigned i, unsigned n)
{
    return static_cast<unsigned>(((rb_mix(key ^ rb_mix(i)) >> 32) * static_cast<unsigned long long>(n)) >> 32);
}

__device__ __forceinline__ void rb_snapshot(long long *rng_state, unsigned long long *snap)
{
    snap[0] = static_cast<unsigned long long>(rng_state[0]);
    snap[1] = static_cast<unsigned long long>(rng_state[1]);
    rng_state[1] = rng_state[1] + 1;   // the next call (the next batch) draws afresh
}

__host__ __device__ inline size_t rb_align(size_t v) { return (v + 255) & ~static_cast<size_t>(255); }

// ================================================================ points
struct PtsArgs {
    int b, p, chunks;
    long long total;
    const float *points;          // (total, 4)
    const long long *offsets;     // (b + 1)
    const double *m, *p2;         // (b, 12) each: R0_rect . Tr_velo_to_cam rows 0..2, P2
    const int *wh, *flip;         // (b, 2), (b)
    unsigned char *cls;           // workspace (total): 0 out of view, 1 near, 2 far
    int *cnt;                     // workspace (b, chunks, 2): near / far per block, then their exclusive offsets
    int *info;                    // workspace (b, 4): n_near, n_far, n
    int *kept;                    // workspace (total): frame start + kept rank -> raw row
    unsigned long long *snap;     // workspace: base seed, call number of this call
    float *xyz, *inten;
    int *src, *status;
};

__device__ __forceinline__ void rb_frame_range(const PtsArgs &a, int f, long long &start, long long &n)
{
    long long s = a.offsets[f], e = a.offsets[f + 1];
    s = s < 0 ? 0 : (s > a.total ? a.total : s);
    e = e < s ? s : (e > a.total ? a.total : e);
    start = s;
    n = e - s;
}

// the rect-frame position of a raw row (fp64, the order kitti_io.lidar_to_rect / project_to_image write)
__device__ __forceinline__ void rb_rect(const double *m, const float *pt, double &x, double &y, double &z)
{
    const double px = pt[0], py = pt[1], pz = pt[2];
    x = m[0] * px + m[1] * py + m[2] * pz + m[3];
    y = m[4] * px + m[5] * py + m[6] * pz + m[7];
    z = m[8] * px + m[9] * py + m[10] * pz + m[11];
}

__global__ __launch_bounds__(kRbThreads) void rb_classify_kernel(PtsArgs a, long long *__restrict__ rng_state)
{
    const int f = blockIdx.y, t = threadIdx.x;
    if (blockIdx.x == 0 && f == 0 && t == 0 && rng_state) rb_snapshot(rng_state, a.snap);
    long long start, n;
    rb_frame_range(a, f, start, n);
    const long long i = static_cast<long long>(blockIdx.x) * kRbThreads + t;
    int c = 0;
    if (i < n) {
        double x, y, z;
        rb_rect(a.m + 12 * f, a.points + (start + i) * 4, x, y, z);
        if (z > 0.0) {
            const double *p = a.p2 + 12 * f;
            const double u = p[0] * x + p[1] * y + p[2] * z + p[3];
            const double v = p[4] * x + p[5] * y + p[6] * z + p[7];
            const double w = p[8] * x + p[9] * y + p[10] * z + p[11];
            const double pu = u / w, pv = v / w;
            if (pu > 0.0 && pu < static_cast<double>(a.wh[2 * f]) && pv > 0.0 && pv < static_cast<double>(a.wh[2 * f + 1]))
                c = z < kRbFarDepth ? 1 : 2;
        }
        a.cls[start + i] = static_cast<unsigned char>(c);
    }
    const int near = __syncthreads_count(c == 1), far = __syncthreads_count(c == 2);
    if (t == 0) {
        int *o = a.cnt + (static_cast<long long>(f) * a.chunks + blockIdx.x) * 2;
        o[0] = near;
        o[1] = far;
    }
}

__global__ __launch_bounds__(kRbThreads) void rb_scan_kernel(PtsArgs a)
{
    __shared__ int s_n[kRbThreads], s_f[kRbThreads];
    const int f = blockIdx.x, t = threadIdx.x;
    int carry_n = 0, carry_f = 0;
    int *cnt = a.cnt + static_cast<long long>(f) * a.chunks * 2;
    for (int base = 0; base < a.chunks; base += kRbThreads) {
        const int c = base + t;
        const int vn = c < a.chunks ? cnt[2 * c] : 0, vf = c < a.chunks ? cnt[2 * c + 1] : 0;
        s_n[t] = vn; s_f[t] = vf;
        __syncthreads();
        for (int d = 1; d < kRbThreads; d <<= 1) {   // inclusive Hillis-Steele scan
            const int an = t >= d ? s_n[t - d] : 0, af = t >= d ? s_f[t - d] : 0;
            __syncthreads();
            s_n[t] += an; s_f[t] += af;
            __syncthreads();
        }
        if (c < a.chunks) { cnt[2 * c] = carry_n + s_n[t] - vn; cnt[2 * c + 1] = carry_f + s_f[t] - vf; }
        carry_n += s_n[kRbThreads - 1];
        carry_f += s_f[kRbThreads - 1];
        __syncthreads();
    }
    if (t == 0) {
        const int n = carry_n + carry_f;
        a.info[4 * f + 0] = carry_n;
        a.info[4 * f + 1] = carry_f;
        a.info[4 * f + 2] = n;
        a.status[f] = (n == 0 ? HF_RPN_BATCH_EMPTY : 0) | (a.p < n && carry_f > a.p ? HF_RPN_BATCH_TOO_MANY_FAR : 0);
    }
}

// output slot `slot` of frame f := raw row `row` (frame-local index `local`)
__device__ __forceinline__ void rb_write(const PtsArgs &a, int f, unsigned slot, long long row, long long local)
{
    double x, y, z;
    const float *pt = a.points + row * 4;
    rb_rect(a.m + 12 * f, pt, x, y, z);
    const long long o = static_cast<long long>(f) * a.p + slot;
    const float fx = static_cast<float>(x);
    a.xyz[3 * o + 0] = a.flip[f] ? -fx : fx;   // kitti_aug.flip_points
    a.xyz[3 * o + 1] = static_cast<float>(y);
    a.xyz[3 * o + 2] = static_cast<float>(z);
    a.inten[o] = pt[3] - 0.5f;
    a.src[o] = static_cast<int>(local);
}

__global__ __launch_bounds__(kRbThreads) void rb_place_kernel(PtsArgs a)
{
    __shared__ int s_wn[kRbThreads / kWave], s_wf[kRbThreads / kWave];
    const int f = blockIdx.y, t = threadIdx.x, lane = t & (kWave - 1), wv = t / kWave;
    long long start, n_raw;
    rb_frame_range(a, f, start, n_raw);
    const long long i = static_cast<long long>(blockIdx.x) * kRbThreads + t;
    const int c = i < n_raw ? a.cls[start + i] : 0;
    const unsigned long long bn = __ballot(c == 1), bf = __ballot(c == 2);
    const unsigned long long below = (1ull << lane) - 1ull;
    if (lane == 0) { s_wn[wv] = __popcll(bn); s_wf[wv] = __popcll(bf); }
    __syncthreads();
    if (c == 0) return;
    const int *cnt = a.cnt + (static_cast<long long>(f) * a.chunks + blockIdx.x) * 2;
    int rn = cnt[0] + __popcll(bn & below), rf = cnt[1] + __popcll(bf & below);
    for (int w = 0; w < wv; ++w) { rn += s_wn[w]; rf += s_wf[w]; }
    const int nn = a.info[4 * f + 0], nf = a.info[4 * f + 1], n = a.info[4 * f + 2];
    const unsigned kept = static_cast<unsigned>(rn + rf);   // near + far points before this one: its rank among the kept
    a.kept[start + kept] = static_cast<int>(i);
    const RbPerm shuffle = rb_perm(rb_key(a.snap, f, kRbShuffle), static_cast<unsigned>(a.p));
    const long long row = start + i;
    if (a.p < n) {
        if (nf > a.p) {                       // more far points than P: a random P of them (the reference fails here)
            if (c == 2) {
                const unsigned q = rb_apply(rb_perm(rb_key(a.snap, f, kRbFar), static_cast<unsigned>(nf)), static_cast<unsigned>(rf));
                if (q < static_cast<unsigned>(a.p)) rb_write(a, f, rb_apply(shuffle, q), row, i);
            }
        } else {
            const unsigned m = static_cast<unsigned>(a.p - nf);   // near points drawn without replacement
            if (c == 1) {
                const unsigned q = rb_apply(rb_perm(rb_key(a.snap, f, kRbNear), static_cast<unsigned>(nn)), static_cast<unsigned>(rn));
                if (q < m) rb_write(a, f, rb_apply(shuffle, q), row, i);
            } else {
                rb_write(a, f, rb_apply(shuffle, m + static_cast<unsigned>(rf)), row, i);   // every far point
            }
        }
    } else {
        rb_write(a, f, rb_apply(shuffle, kept), row, i);          // every point once
        const int extra = a.p - n;
        if (extra > 0 && a.p <= 2ll * n) {                           // extra draws without replacement
            const unsigned q = rb_apply(rb_perm(rb_key(a.snap, f, kRbExtra), static_cast<unsigned>(n)), kept);
            if (q < static_cast<unsigned>(extra)) rb_write(a, f, rb_apply(shuffle, static_cast<unsigned>(n) + q), row, i);
        }
    }
}

__global__ __launch_bounds__(kRbThreads) void rb_fill_kernel(PtsArgs a)
{
    const int f = blockIdx.y;
    const int j = blockIdx.x * kRbThreads + threadIdx.x;
    if (j >= a.p) return;
    const int n = a.info[4 * f + 2];
    if (n == 0) {   // nothing in view (the reference fails here): zeros
        const long long o = static_cast<long long>(f) * a.p + j;
        a.xyz[3 * o] = 0.0f; a.xyz[3 * o + 1] = 0.0f; a.xyz[3 * o + 2] = 0.0f;
        a.inten[o] = 0.0f;
        a.src[o] = -1;
        return;
    }
    if (a.p <= 2ll * n || j >= a.p - n) return;
    // extra draw j with replacement (P > 2 n): a uniform kept point
    long long start, n_raw;
    rb_frame_range(a, f, start, n_raw);
    const unsigned k = rb_index(rb_key(a.snap, f, kRbDraw), static_cast<unsigned>(j), static_cast<unsigned>(n));
    const long long local = a.kept[start + k];
    const RbPerm shuffle = rb_perm(rb_key(a.snap, f, kRbShuffle), static_cast<unsigned>(a.p));
    rb_write(a, f, rb_apply(shuffle, static_cast<unsigned>(n + j)), start + local, local);
}

static size_t rb_pts_cls_offset() { return 256; }
static size_t rb_pts_cnt_offset(long long total) { return rb_pts_cls_offset() + rb_align(static_cast<size_t>(total)); }
static size_t rb_pts_info_offset(int b, long long total, int chunks)
{
    return rb_pts_cnt_offset(total) + rb_align(sizeof(int) * 2 * static_cast<size_t>(b) * chunks);
}
static size_t rb_pts_kept_offset(int b, long long total, int chunks) { return rb_pts_info_offset(b, total, chunks) + rb_align(sizeof(int) * 4 * static_cast<size_t>(b)); }
static size_t rb_pts_bytes(int b, long long total, int chunks) { return rb_pts_kept_offset(b, total, chunks) + rb_align(sizeof(int) * static_cast<size_t>(total)); }

static bool rb_pts_shape_ok(int b, long long total, long long max_frame)
{
    return b >= 0 && b <= kRbMaxB && total >= 0 && max_frame >= 0 && max_frame <= kRbMaxFrame && max_frame <= total;
}

// ================================================================ labels
struct RbBox {
    double u[3], v[3], w[3], lo[3], hi[3];
};

// obj_utils.is_point_inside over the corners of box_8c_encoder.np_box_3d_to_box_8co: the corner templates are float32
// (l / 2, w / 2, h), the rotation and the sums fp64; P1 = (l/2, 0, w/2), P2 = (l/2, 0, -w/2), P4 = (-l/2, 0, w/2),
// P5 = (l/2, -h, w/2) before rotation by ry about y and the shift to (x, y, z)
__device__ void rb_box_prepare(double x, double y, double z, double l, double w, double h, double ry, RbBox &o)
{
    const double hl = static_cast<float>(l / 2.0), hw = static_cast<float>(w / 2.0), hh = static_cast<float>(h);
    const double c = cos(ry), s = sin(ry);
    const double tx[4] = { hl, hl, -hl, hl }, ty[4] = { 0.0, 0.0, 0.0, -hh }, tz[4] = { hw, -hw, hw, hw };
    double pc[4][3];
    for (int k = 0; k < 4; ++k) {   // [tx ty tz] @ [[c, 0, -s], [0, 1, 0], [s, 0, c]] + location
        pc[k][0] = x + (tx[k] * c + ty[k] * 0.0 + tz[k] * s);
        pc[k][1] = y + (tx[k] * 0.0 + ty[k] * 1.0 + tz[k] * 0.0);
        pc[k][2] = z + (tx[k] * -s + ty[k] * 0.0 + tz[k] * c);
    }
    for (int d = 0; d < 3; ++d) {
        o.u[d] = pc[1][d] - pc[0][d];
        o.v[d] = pc[2][d] - pc[0][d];
        o.w[d] = pc[3][d] - pc[0][d];
    }
    const double *e[3] = { o.u, o.v, o.w };
    for (int q = 0; q < 3; ++q) {
        o.lo[q] = e[q][0] * pc[0][0] + e[q][1] * pc[0][1] + e[q][2] * pc[0][2];
        o.hi[q] = e[q][0] * pc[q + 1][0] + e[q][1] * pc[q + 1][1] + e[q][2] * pc[q + 1][2];
    }
}

__device__ __forceinline__ bool rb_inside(const RbBox &b, double px, double py, double pz)
{
    const double du = b.u[0] * px + b.u[1] * py + b.u[2] * pz;
    const double dv = b.v[0] * px + b.v[1] * py + b.v[2] * pz;
    const double dw = b.w[0] * px + b.w[1] * py + b.w[2] * pz;
    return b.lo[0] < du && du < b.hi[0] && b.lo[1] < dv && dv < b.hi[1] && b.lo[2] < dw && dw < b.hi[2];
}

__global__ __launch_bounds__(kRbThreads) void rb_labels_kernel(int p, int g, const float *__restrict__ xyz, const float *__restrict__ boxes,
                                                               const int *__restrict__ classes, const int *__restrict__ gt_count,
                                                               double expand, int *__restrict__ label_cls, float *__restrict__ label_reg)
{
    __shared__ RbBox s_box[kRbMaxG], s_ext[kRbMaxG];
    const int f = blockIdx.y, t = threadIdx.x;
    const int ng = min(max(gt_count[f], 0), g);
    const float *bx = boxes + static_cast<long long>(f) * g * 7;
    for (int k = t; k < ng; k += kRbThreads) {
        const float *q = bx + 7 * k;
        rb_box_prepare(q[0], q[1], q[2], q[3], q[4], q[5], q[6], s_box[k]);
        // the enlarged box: l, w, h + 2 expand, y + expand (the bottom moves down by expand, the top up by expand)
        rb_box_prepare(q[0], static_cast<double>(q[1]) + expand, q[2], static_cast<double>(q[3]) + expand * 2.0,
                       static_cast<double>(q[4]) + expand * 2.0, static_cast<double>(q[5]) + expand * 2.0, q[6], s_ext[k]);
    }
    __syncthreads();
    const int j = blockIdx.x * kRbThreads + t;
    if (j >= p) return;
    const long long o = static_cast<long long>(f) * p + j;
    const double px = xyz[3 * o], py = xyz[3 * o + 1], pz = xyz[3 * o + 2];
    int cls = 0, reg = -1;
    for (int k = 0; k < ng; ++k) {
        const bool in = rb_inside(s_box[k], px, py, pz), ex = rb_inside(s_ext[k], px, py, pz);
        if (in) { cls = classes[static_cast<long long>(f) * g + k]; reg = k; }   // a later box overwrites an earlier one
        if (in != ex) cls = -1;                                                // the ring (xor): ignored
    }
    label_cls[o] = cls;
    for (int d = 0; d < 7; ++d) label_reg[7 * o + d] = reg >= 0 ? bx[7 * reg + d] : 0.0f;   // the box of the last containing box
}

// ================================================================ image
struct ImgArgs {
    int b, chunks, out_h, out_w;
    long long total_bytes;
    const unsigned char *img;     // packed HWC RGB
    const long long *offsets;     // (b) byte offset of each frame
    const int *wh, *flip, *jitter;
    unsigned long long *snap, *partial;   // workspace: RNG snapshot; (b, chunks, 9) integer sums
    double *noise, *stats;        // (b, 3); optional (b, 21)
    float *out;                   // (b, out_h, out_w, 3)
};

// the frame's size when its bytes lie inside the buffer, else 0 pixels
__device__ __forceinline__ long long rb_img_pixels(const ImgArgs &a, int f, int &w, int &h, long long &off)
{
    w = a.wh[2 * f]; h = a.wh[2 * f + 1]; off = a.offsets[f];
    if (w < 1 || h < 1 || w > kRbImgMaxSide || h > kRbImgMaxSide) return 0;
    const long long n = static_cast<long long>(w) * h;
    if (n > kRbImgMaxPixels || off < 0 || off + 3 * n > a.total_bytes) return 0;
    return n;
}

__global__ __launch_bounds__(kRbThreads) void rb_img_sums_kernel(ImgArgs a, long long *__restrict__ rng_state)
{
    __shared__ unsigned long long red[9][kRbThreads];
    const int f = blockIdx.y, t = threadIdx.x;
    if (blockIdx.x == 0 && f == 0 && t == 0 && rng_state) rb_snapshot(rng_state, a.snap);
    if (!a.jitter[f]) return;   // uniform over the block
    int w, h;
    long long off;
    const long long n = rb_img_pixels(a, f, w, h, off);
    unsigned long long s[9] = { 0, 0, 0, 0, 0, 0, 0, 0, 0 };
    const long long base = static_cast<long long>(blockIdx.x) * kRbThreads * kRbImgPixPerThread;
    for (int k = 0; k < kRbImgPixPerThread; ++k) {
        const long long i = base + static_cast<long long>(k) * kRbThreads + t;
        if (i >= n) break;
        const unsigned char *px = a.img + off + 3 * i;
        const unsigned long long r = px[0], g = px[1], bb = px[2];
        s[0] += r; s[1] += g; s[2] += bb;
        s[3] += r * r; s[4] += r * g; s[5] += r * bb; s[6] += g * g; s[7] += g * bb; s[8] += bb * bb;
    }
    for (int q = 0; q < 9; ++q) red[q][t] = s[q];
    __syncthreads();
    for (int d = kRbThreads / 2; d > 0; d >>= 1) {
        if (t < d)
            for (int q = 0; q < 9; ++q) red[q][t] += red[q][t + d];
        __syncthreads();
    }
    if (t < 9) a.partial[(static_cast<long long>(f) * a.chunks + blockIdx.x) * 9 + t] = red[t][0];
}

// 3x3 symmetric eigendecomposition, cyclic Jacobi (Numerical Recipes' rotation); eigenvalues ascending, vectors in columns
__device__ void rb_jacobi3(double a[3][3], double e[3], double v[3][3])
{
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) v[i][j] = i == j ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 32; ++sweep) {
        const double off = fabs(a[0][1]) + fabs(a[0][2]) + fabs(a[1][2]);
        if (off == 0.0) break;
        const int pp[3] = { 0, 0, 1 }, qq[3] = { 1, 2, 2 };
        for (int r = 0; r < 3; ++r) {
            const int p = pp[r], q = qq[r];
            if (a[p][q] == 0.0) continue;
            const double theta = (a[q][q] - a[p][p]) / (2.0 * a[p][q]);
            const double tt = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
            const double c = 1.0 / sqrt(tt * tt + 1.0), s = tt * c;
            for (int k = 0; k < 3; ++k) {
                const double akp = a[k][p], akq = a[k][q];
                a[k][p] = c * akp - s * akq;
                a[k][q] = s * akp + c * akq;
            }
            for (int k = 0; k < 3; ++k) {
                const double apk = a[p][k], aqk = a[q][k];
                a[p][k] = c * apk - s * aqk;
                a[q][k] = s * apk + c * aqk;
            }
            a[p][q] = 0.0;
            a[q][p] = 0.0;
            for (int k = 0; k < 3; ++k) {
                const double vkp = v[k][p], vkq = v[k][q];
                v[k][p] = c * vkp - s * vkq;
                v[k][q] = s * vkp + c * vkq;
            }
        }
    }
    int ord[3] = { 0, 1, 2 };
    for (int i = 0; i < 3; ++i)
        for (int j = i + 1; j < 3; ++j)
            if (a[ord[j]][ord[j]] < a[ord[i]][ord[i]]) { const int tmp = ord[i]; ord[i] = ord[j]; ord[j] = tmp; }
    double vs[3][3];
    for (int j = 0; j < 3; ++j) {
        e[j] = a[ord[j]][ord[j]];
        for (int i = 0; i < 3; ++i) vs[i][j] = v[i][ord[j]];
    }
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) v[i][j] = vs[i][j];
}

__global__ __launch_bounds__(64) void rb_img_pca_kernel(ImgArgs a)
{
    __shared__ unsigned long long red[9][64];
    const int f = blockIdx.x, t = threadIdx.x;
    double *nz = a.noise + 3 * f;
    int w, h;
    long long off;
    const long long n = rb_img_pixels(a, f, w, h, off);
    if (!a.jitter[f] || n < 2) {
        if (t == 0) {
            nz[0] = 0.0; nz[1] = 0.0; nz[2] = 0.0;
            if (a.stats)
                for (int q = 0; q < 21; ++q) a.stats[21 * f + q] = 0.0;
        }
        return;
    }
    unsigned long long s[9] = { 0, 0, 0, 0, 0, 0, 0, 0, 0 };
    const int used = min(a.chunks, static_cast<int>((n + kRbThreads * kRbImgPixPerThread - 1) / (kRbThreads * kRbImgPixPerThread)));
    for (int c = t; c < used; c += 64)
        for (int q = 0; q < 9; ++q) s[q] += a.partial[(static_cast<long long>(f) * a.chunks + c) * 9 + q];
    for (int q = 0; q < 9; ++q) red[q][t] = s[q];
    __syncthreads();
    if (t != 0) return;
    for (int q = 0; q < 9; ++q) {
        unsigned long long acc = 0;
        for (int k = 0; k < 64; ++k) acc += red[q][k];   // integers: the order does not matter
        s[q] = acc;
    }
    // np.cov(x / 255, ddof 1) = (N sum(x_i x_j) - sum(x_i) sum(x_j)) / (N (N - 1) 255^2), the numerator exact in int64
    const long long N = n;
    const int ii[6] = { 0, 0, 0, 1, 1, 2 }, jj[6] = { 0, 1, 2, 1, 2, 2 };
    double cov[3][3];
    const double den = static_cast<double>(N) * static_cast<double>(N - 1) * (255.0 * 255.0);
    for (int q = 0; q < 6; ++q) {
        const long long num = N * static_cast<long long>(s[3 + q]) - static_cast<long long>(s[ii[q]]) * static_cast<long long>(s[jj[q]]);
        cov[ii[q]][jj[q]] = cov[jj[q]][ii[q]] = static_cast<double>(num) / den;
    }
    double work[3][3], e[3], v[3][3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) work[i][j] = cov[i][j];
    rb_jacobi3(work, e, v);
    // pca = sqrt(e) * V (column j scaled by sqrt(e_j); rounding can leave e_j slightly below 0: taken as 0);
    // noise_i = sum_j pca[i][j] * 0.1 N_j (kitti_aug.add_pca_jitter), the normals by Box-Muller from the counter hash
    const unsigned long long key = rb_key(a.snap, f, kRbNormal);
    double mag[3];
    for (int j = 0; j < 3; ++j) {
        const double u1 = (static_cast<double>(rb_mix(key ^ rb_mix(2 * j)) >> 11) + 1.0) * (1.0 / 9007199254740992.0);   // (0, 1]
        const double u2 = static_cast<double>(rb_mix(key ^ rb_mix(2 * j + 1)) >> 11) * (1.0 / 9007199254740992.0);
        mag[j] = sqrt(-2.0 * log(u1)) * cos(2.0 * M_PI * u2) * 0.1;
    }
    for (int i = 0; i < 3; ++i) {
        double acc = 0.0;
        for (int j = 0; j < 3; ++j) acc = acc + sqrt(e[j] > 0.0 ? e[j] : 0.0) * v[i][j] * mag[j];
        nz[i] = acc;
    }
    if (a.stats) {
        double *st = a.stats + 21 * f;
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) { st[3 * i + j] = cov[i][j]; st[12 + 3 * i + j] = v[i][j]; }
        for (int j = 0; j < 3; ++j) st[9 + j] = e[j];
    }
}

// cv2 INTER_LINEAR geometry of one axis: f = (d + 0.5) * (S / D) - 0.5 in fp64 rounded to fp32, s = floor(f), weight f - s;
// s < 0 -> (0, 0), s >= S - 1 -> (S - 1, 0)
__device__ __forceinline__ void rb_axis(int d, double scale, int size, int &s0, int &s1, float &wt)
{
    float fv = static_cast<float>((d + 0.5) * scale - 0.5);
    const float fl = floorf(fv);
    int s = static_cast<int>(fl);
    fv = fv - fl;
    if (s < 0) { fv = 0.0f; s = 0; }
    if (s >= size - 1) { fv = 0.0f; s = size - 1; }
    s0 = s;
    s1 = s + 1 < size ? s + 1 : size - 1;
    wt = fv;
}

// one source value after kitti_aug.add_pca_jitter: trunc(clip(f64(f32(x) / 255) + noise, 0, 1) * 255)
__device__ __forceinline__ float rb_jit(unsigned char x, double noise)
{
    double v = static_cast<double>(static_cast<float>(x) / 255.0f) + noise;
    v = v < 0.0 ? 0.0 : (v > 1.0 ? 1.0 : v);
    return static_cast<float>(static_cast<int>(v * 255.0));
}

__global__ __launch_bounds__(kRbThreads) void rb_img_resize_kernel(ImgArgs a)
{
    const int f = blockIdx.y;
    const long long idx = static_cast<long long>(blockIdx.x) * kRbThreads + threadIdx.x;
    const long long plane = static_cast<long long>(a.out_h) * a.out_w;
    if (idx >= plane) return;
    float *o = a.out + (static_cast<long long>(f) * plane + idx) * 3;
    int w, h;
    long long off;
    if (rb_img_pixels(a, f, w, h, off) == 0) {
        o[0] = 0.0f; o[1] = 0.0f; o[2] = 0.0f;
        return;
    }
    const int dy = static_cast<int>(idx / a.out_w), dx = static_cast<int>(idx % a.out_w);
    int x0, x1, y0, y1;
    float wx, wy;
    rb_axis(dx, static_cast<double>(w) / a.out_w, w, x0, x1, wx);
    rb_axis(dy, static_cast<double>(h) / a.out_h, h, y0, y1, wy);
    if (a.flip[f]) { x0 = w - 1 - x0; x1 = w - 1 - x1; }   // kitti_aug.flip_image: the source column mirrored
    const bool jit = a.jitter[f] != 0;
    const unsigned char *src = a.img + off;
    const long long p00 = 3 * (static_cast<long long>(y0) * w + x0), p01 = 3 * (static_cast<long long>(y0) * w + x1);
    const long long p10 = 3 * (static_cast<long long>(y1) * w + x0), p11 = 3 * (static_cast<long long>(y1) * w + x1);
    const float ux = 1.0f - wx, uy = 1.0f - wy;
    for (int c = 0; c < 3; ++c) {
        const double nz = jit ? a.noise[3 * f + c] : 0.0;
        float v00 = src[p00 + c], v01 = src[p01 + c], v10 = src[p10 + c], v11 = src[p11 + c];
        if (jit) { v00 = rb_jit(src[p00 + c], nz); v01 = rb_jit(src[p01 + c], nz); v10 = rb_jit(src[p10 + c], nz); v11 = rb_jit(src[p11 + c], nz); }
        const float r = (v00 * ux + v01 * wx) * uy + (v10 * ux + v11 * wx) * wy;
        o[c] = fminf(fmaxf(rintf(r), 0.0f), 255.0f);
    }
}

static bool rb_img_shape_ok(int b, long long max_pixels, int out_h, int out_w)
{
    return b >= 0 && b <= kRbMaxB && max_pixels >= 0 && max_pixels <= kRbImgMaxPixels && out_h >= 1 && out_h <= kRbImgMaxSide &&
           out_w >= 1 && out_w <= kRbImgMaxSide;
}
static int rb_img_chunks(long long max_pixels) { return max_pixels > 0 ? div_up(max_pixels, kRbThreads * kRbImgPixPerThread) : 1; }
static size_t rb_img_bytes(int b, int chunks) { return 256 + rb_align(sizeof(unsigned long long) * 9 * static_cast<size_t>(b) * chunks); }

}  // namespace hf

using namespace hf;

HF_API size_t hf_rpn_batch_points_workspace(int b, long long total, long long max_frame_points)
{
    if (!rb_pts_shape_ok(b, total, max_frame_points)) return 0;
    return rb_pts_bytes(b, total, max_frame_points > 0 ? div_up(max_frame_points, kRbThreads) : 1);
}

HF_API int hf_rpn_batch_points(int b, int p, long long total, long long max_frame_points, const float *points,
                               const long long *offsets, const double *velo_to_rect, const double *p2, const int *image_wh,
                               const int *flip, long long *rng_state, float *xyz, float *intensity, int *src_index, int *status,
                               void *workspace, size_t workspace_bytes, hf_stream_t stream)
{
    if (!rb_pts_shape_ok(b, total, max_frame_points) || p < 1 || p > kRbMaxP) return HF_EINVAL;
    if (b == 0) return HF_OK;
    if ((total > 0 && !points) || !offsets || !velo_to_rect || !p2 || !image_wh || !flip || !rng_state || !xyz || !intensity ||
        !src_index || !status)
        return HF_EINVAL;
    const int chunks = max_frame_points > 0 ? div_up(max_frame_points, kRbThreads) : 1;
    if (!workspace || workspace_bytes < rb_pts_bytes(b, total, chunks)) return HF_EWORKSPACE;
    unsigned char *ws = static_cast<unsigned char *>(workspace);
    PtsArgs a;
    a.b = b; a.p = p; a.chunks = chunks; a.total = total;
    a.points = points; a.offsets = offsets; a.m = velo_to_rect; a.p2 = p2; a.wh = image_wh; a.flip = flip;
    a.snap = reinterpret_cast<unsigned long long *>(ws);
    a.cls = ws + rb_pts_cls_offset();
    a.cnt = reinterpret_cast<int *>(ws + rb_pts_cnt_offset(total));
    a.info = reinterpret_cast<int *>(ws + rb_pts_info_offset(b, total, chunks));
    a.kept = reinterpret_cast<int *>(ws + rb_pts_kept_offset(b, total, chunks));
    a.xyz = xyz; a.inten = intensity; a.src = src_index; a.status = status;
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(rb_classify_kernel, dim3(chunks, b), dim3(kRbThreads), 0, st, a, rng_state);
    hipLaunchKernelGGL(rb_scan_kernel, dim3(b), dim3(kRbThreads), 0, st, a);
    hipLaunchKernelGGL(rb_place_kernel, dim3(chunks, b), dim3(kRbThreads), 0, st, a);
    hipLaunchKernelGGL(rb_fill_kernel, dim3(div_up(p, kRbThreads), b), dim3(kRbThreads), 0, st, a);
    return launch_status();
}

HF_API int hf_rpn_point_labels(int b, int p, int g, const float *xyz, const float *boxes, const int *classes, const int *gt_count,
                               float expand, int *label_cls, float *label_reg, hf_stream_t stream)
{
    if (b < 0 || b > kRbMaxB || p < 1 || p > kRbMaxP || g < 0 || g > kRbMaxG || !(expand >= 0.0f && expand < 1e3f)) return HF_EINVAL;
    if (b == 0) return HF_OK;
    if (!xyz || !gt_count || (g > 0 && (!boxes || !classes)) || !label_cls || !label_reg) return HF_EINVAL;
    hipLaunchKernelGGL(rb_labels_kernel, dim3(div_up(p, kRbThreads), b), dim3(kRbThreads), 0, as_stream(stream), p, g, xyz, boxes,
                       classes, gt_count, static_cast<double>(expand), label_cls, label_reg);
    return launch_status();
}

HF_API size_t hf_rpn_batch_image_workspace(int b, long long max_pixels)
{
    if (!rb_img_shape_ok(b, max_pixels, 1, 1)) return 0;
    return rb_img_bytes(b, rb_img_chunks(max_pixels));
}

HF_API int hf_rpn_batch_image(int b, long long max_pixels, long long total_bytes, const unsigned char *images,
                              const long long *image_offsets, const int *image_wh, const int *flip, const int *jitter, int out_h,
                              int out_w, long long *rng_state, float *image, double *noise, double *pca_stats, void *workspace,
                              size_t workspace_bytes, hf_stream_t stream)
{
    if (!rb_img_shape_ok(b, max_pixels, out_h, out_w) || total_bytes < 0) return HF_EINVAL;
    if (b == 0) return HF_OK;
    if ((total_bytes > 0 && !images) || !image_offsets || !image_wh || !flip || !jitter || !rng_state || !image || !noise)
        return HF_EINVAL;
    const int chunks = rb_img_chunks(max_pixels);
    if (!workspace || workspace_bytes < rb_img_bytes(b, chunks)) return HF_EWORKSPACE;
    unsigned char *ws = static_cast<unsigned char *>(workspace);
    ImgArgs a;
    a.b = b; a.chunks = chunks; a.out_h = out_h; a.out_w = out_w; a.total_bytes = total_bytes;
    a.img = images; a.offsets = image_offsets; a.wh = image_wh; a.flip = flip; a.jitter = jitter;
    a.snap = reinterpret_cast<unsigned long long *>(ws);
    a.partial = reinterpret_cast<unsigned long long *>(ws + 256);
    a.noise = noise; a.stats = pca_stats; a.out = image;
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(rb_img_sums_kernel, dim3(chunks, b), dim3(kRbThreads), 0, st, a, rng_state);
    hipLaunchKernelGGL(rb_img_pca_kernel, dim3(b), dim3(64), 0, st, a);
    hipLaunchKernelGGL(rb_img_resize_kernel, dim3(div_up(static_cast<long long>(out_h) * out_w, kRbThreads), b), dim3(kRbThreads), 0, st, a);
    return launch_status();
}
