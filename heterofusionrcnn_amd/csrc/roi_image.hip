// roi_image.hip -- the image half of the second stage's RoI pooling for gfx950 (hf/core/models/rcnn_model.py:433-454, 494-501).
//
//   roi_image_boxes       hf/core/projection.py:35-96 (tf_project_to_image_space) + anchor_projector.reorder_projected_boxes:
//                         the eight corners of a proposal (box_8c_encoder.py:101-185) times P2, divided by depth, their bounding
//                         rectangle in pixels, normalised by [w,h,w,h], and the same as [y1,x1,y2,x2].  Eight lanes per box, one
//                         corner each; min / max over the eight lanes by __shfl_xor.  No clipping and no special case for a corner
//                         behind the camera (the reference has neither); a NaN corner makes the rectangle NaN, as tf.reduce_min.
//   crop_and_resize       tf.image.crop_and_resize, bilinear (TensorFlow's CPU kernel, crop_and_resize_op.cc): c / VEC lanes per
//                         sample, the four corner rows of a sample are read as 16-byte pieces of contiguous runs of c floats.
//   crop_and_resize_grad  the gradient w.r.t. the image: one lane per (sample, channel) dword, four no-return fp32 atomic adds,
//                         contiguous along c (128-byte row segments at c = 32), into a map zero-filled on the stream by
//                         zero_fill_kernel.  Not hipMemsetAsync: a captured memset node of a small map (245 760 bytes) wrote the
//                         zeros on the first replay of its graph and a 16-byte pattern of stale words on every later one, for
//                         hf_project_gather_grad's memset just the same; a kernel node replays what it was given.
//   crop_and_resize_grad_ordered  the same gradient with every pixel's shares added in ascending (sample, tap) order, no fp atomics:
//                         CropGradEntries on the machine of ordered_scatter.h; it writes every row of the map itself.
// All crop kernels form the sample coordinates with the same function, so both directions and both forms take the same in-range decisions
// and nothing is saved between them.  No address is formed from a coordinate or a box index that failed its test.
// Arithmetic: fp32, no contraction, correctly rounded division; expressions in the order of fusion.py's tensor form.
#include <limits.h>
#include <math.h>

#include "hf_common.h"
#include "ordered_scatter.h"

namespace hf {

// min / max that hand a NaN on, whichever side it is on (tf.reduce_min / torch.min)
__device__ __forceinline__ float nan_min(float a, float b) { return (a < b || a != a) ? a : b; }
__device__ __forceinline__ float nan_max(float a, float b) { return (a > b || a != a) ? a : b; }

constexpr int kBoxLanes = 8;   // one lane per corner

__global__ __launch_bounds__(256) void roi_image_boxes_kernel(int n, long long nbox, float w, float h,
                                                              const float *__restrict__ boxes3d, const float *__restrict__ calib,
                                                              float *__restrict__ box_px, float *__restrict__ box_norm,
                                                              float *__restrict__ box_yxyx)
{
    const long long t = blockIdx.x * static_cast<long long>(blockDim.x) + threadIdx.x;
    const long long box = t / kBoxLanes;
    const int k = static_cast<int>(t - box * kBoxLanes);          // corner P1..P8 of box_8c_encoder.py:21-37
    const bool live = box < nbox;
    const long long row = live ? box : nbox - 1;                  // dead lanes of the last wave recompute the last box
    const float *bx = boxes3d + row * 7;
    const float *P = calib + (row / n) * 12;
    const float ry = bx[6];
    const float s = sinf(ry), c = cosf(ry);
    const float hl = bx[3] / 2.0f, hw = bx[4] / 2.0f;
    const float xc = (k & 2) ? -hl : hl;                          // [hl, hl, -hl, -hl, hl, hl, -hl, -hl]
    const float zc = (((k + 1) & 2) ? -hw : hw);                  // [hw, -hw, -hw, hw, hw, -hw, -hw, hw]
    const float yc = (k & 4) ? -bx[5] : 0.0f;                     // [0, 0, 0, 0, -h, -h, -h, -h]
    const float x = c * xc + s * zc + bx[0];
    const float y = yc + bx[1];
    const float z = -s * xc + c * zc + bx[2];
    const float uh = P[0] * x + P[1] * y + P[2] * z + P[3];       // the order of project_point (glue.hip)
    const float vh = P[4] * x + P[5] * y + P[6] * z + P[7];
    const float d = P[8] * x + P[9] * y + P[10] * z + P[11];
    const float u = uh / d, v = vh / d;
    float x1 = u, y1 = v, x2 = u, y2 = v;
#pragma unroll
    for (int m = 1; m < kBoxLanes; m <<= 1) {
        x1 = nan_min(x1, __shfl_xor(x1, m, kBoxLanes));
        y1 = nan_min(y1, __shfl_xor(y1, m, kBoxLanes));
        x2 = nan_max(x2, __shfl_xor(x2, m, kBoxLanes));
        y2 = nan_max(y2, __shfl_xor(y2, m, kBoxLanes));
    }
    if (!live || k != 0) return;
    const float nx1 = x1 / w, ny1 = y1 / h, nx2 = x2 / w, ny2 = y2 / h;
    // dword stores: the outputs carry no alignment promise beyond a float's
    if (box_px) { float *o = box_px + box * 4; o[0] = x1; o[1] = y1; o[2] = x2; o[3] = y2; }
    if (box_norm) { float *o = box_norm + box * 4; o[0] = nx1; o[1] = ny1; o[2] = nx2; o[3] = ny2; }
    if (box_yxyx) { float *o = box_yxyx + box * 4; o[0] = ny1; o[1] = nx1; o[2] = ny2; o[3] = nx2; }
}

// Sample `i` of `crop` along an axis of `size` pixels between the normalised ends a1, a2 (crop_and_resize_op.cc:241-262,
// fusion.image_crop_and_resize): a1 (size-1) + i ((a2-a1) (size-1) / (crop-1)), the centre for crop == 1.
__device__ __forceinline__ float crop_coord(float a1, float a2, int i, int crop, float size_m1)
{
    if (crop > 1) return a1 * size_m1 + static_cast<float>(i) * ((a2 - a1) * size_m1 / static_cast<float>(crop - 1));
    return 0.5f * (a1 + a2) * size_m1;
}

struct CropSample {
    bool ok;              // in range and a valid box index: only then are the fields below meaningful
    long long base;       // element offset of the frame in the image
    int y0, yb, x0, xb;
    float ly, lx;
};

__device__ __forceinline__ CropSample crop_sample(int b, int h, int w, int c, int crop_h, int crop_w, long long r, int i, int j,
                                                  const float *__restrict__ boxes, const int *__restrict__ box_ind)
{
    const float *bx = boxes + r * 4;
    const float hm1 = static_cast<float>(h - 1), wm1 = static_cast<float>(w - 1);
    const float in_y = crop_coord(bx[0], bx[2], i, crop_h, hm1);
    const float in_x = crop_coord(bx[1], bx[3], j, crop_w, wm1);
    const int bi = box_ind[r];
    CropSample s = {};
    s.ok = in_y >= 0.0f && in_y <= hm1 && in_x >= 0.0f && in_x <= wm1 && bi >= 0 && bi < b;   // a NaN fails every comparison
    if (!s.ok) return s;
    const float y0f = floorf(in_y), x0f = floorf(in_x);
    s.y0 = static_cast<int>(y0f);
    s.yb = static_cast<int>(ceilf(in_y));
    s.x0 = static_cast<int>(x0f);
    s.xb = static_cast<int>(ceilf(in_x));
    s.ly = in_y - y0f;
    s.lx = in_x - x0f;
    s.base = static_cast<long long>(bi) * h * w * c;
    return s;
}

// c / VEC lanes per sample
template <int VEC>
__global__ __launch_bounds__(256) void crop_and_resize_kernel(int b, int h, int w, int c, long long nsamples, int crop_h,
                                                              int crop_w, const float *__restrict__ img,
                                                              const float *__restrict__ boxes, const int *__restrict__ box_ind,
                                                              float extrapolation, float *__restrict__ out)
{
    typedef float vec_t __attribute__((ext_vector_type(VEC)));
    const int cv = c / VEC;
    const long long total = nsamples * cv;
    for (long long e = blockIdx.x * static_cast<long long>(blockDim.x) + threadIdx.x; e < total;
         e += static_cast<long long>(gridDim.x) * blockDim.x) {
        const long long smp = e / cv;
        const int l = static_cast<int>(e - smp * cv) * VEC;
        const long long ri = smp / crop_w;
        const int j = static_cast<int>(smp - ri * crop_w);
        const long long r = ri / crop_h;
        const int i = static_cast<int>(ri - r * crop_h);
        const CropSample s = crop_sample(b, h, w, c, crop_h, crop_w, r, i, j, boxes, box_ind);
        vec_t v;
        if (s.ok) {
            const float *top_row = img + s.base + static_cast<long long>(s.y0) * w * c + l;
            const float *bot_row = img + s.base + static_cast<long long>(s.yb) * w * c + l;
            const long long o0 = static_cast<long long>(s.x0) * c, ob = static_cast<long long>(s.xb) * c;
            const vec_t tl = *reinterpret_cast<const vec_t *>(top_row + o0), tr = *reinterpret_cast<const vec_t *>(top_row + ob);
            const vec_t bl = *reinterpret_cast<const vec_t *>(bot_row + o0), br = *reinterpret_cast<const vec_t *>(bot_row + ob);
            const vec_t top = tl + (tr - tl) * s.lx;
            const vec_t bot = bl + (br - bl) * s.lx;
            v = top + (bot - top) * s.ly;
        } else {
            if constexpr (VEC == 1) v = extrapolation;
            else v = vec_t{ extrapolation, extrapolation, extrapolation, extrapolation };
        }
        *reinterpret_cast<vec_t *>(out + smp * c + l) = v;
    }
}

// one lane per (sample, channel): the four adds of a wave are runs of min(c, 64) contiguous floats
__global__ __launch_bounds__(256) void crop_and_resize_grad_kernel(int b, int h, int w, int c, long long nsamples, int crop_h,
                                                                   int crop_w, const float *__restrict__ grad_out,
                                                                   const float *__restrict__ boxes,
                                                                   const int *__restrict__ box_ind, float *__restrict__ grad_img)
{
    const long long total = nsamples * c;
    for (long long e = blockIdx.x * static_cast<long long>(blockDim.x) + threadIdx.x; e < total;
         e += static_cast<long long>(gridDim.x) * blockDim.x) {
        const long long smp = e / c;
        const int l = static_cast<int>(e - smp * c);
        const long long ri = smp / crop_w;
        const int j = static_cast<int>(smp - ri * crop_w);
        const long long r = ri / crop_h;
        const int i = static_cast<int>(ri - r * crop_h);
        const CropSample s = crop_sample(b, h, w, c, crop_h, crop_w, r, i, j, boxes, box_ind);
        if (!s.ok) continue;
        const float g = grad_out[e];
        const float dtop = (1.0f - s.ly) * g, dbot = s.ly * g;
        float *top_row = grad_img + s.base + static_cast<long long>(s.y0) * w * c + l;
        float *bot_row = grad_img + s.base + static_cast<long long>(s.yb) * w * c + l;
        const long long o0 = static_cast<long long>(s.x0) * c, ob = static_cast<long long>(s.xb) * c;
        atomicAdd(top_row + o0, (1.0f - s.lx) * dtop);
        atomicAdd(top_row + ob, s.lx * dtop);
        atomicAdd(bot_row + o0, (1.0f - s.lx) * dbot);
        atomicAdd(bot_row + ob, s.lx * dbot);
    }
}

// the entries of crop_and_resize_grad for ordered_scatter.h: entry e = sample * 4 + tap, taps tl, tr, bl, br; the sample
// coordinates from crop_sample and the shares in the arithmetic of crop_and_resize_grad_kernel
struct CropGradEntries {
    int b, h, w, c, crop_h, crop_w;
    const float *grad_out, *boxes;
    const int *box_ind;
    __device__ __forceinline__ CropSample sample(int smp) const
    {
        const int ri = smp / crop_w, j = smp - ri * crop_w;
        const int r = ri / crop_h, i = ri - r * crop_h;
        return crop_sample(b, h, w, c, crop_h, crop_w, r, i, j, boxes, box_ind);
    }
    __device__ __forceinline__ int key(int e) const
    {
        const int smp = e >> 2, tap = e & 3;
        const CropSample s = sample(smp);
        if (!s.ok) return -1;
        const int bi = box_ind[smp / (crop_w * crop_h)];
        return (bi * h + (tap & 2 ? s.yb : s.y0)) * w + (tap & 1 ? s.xb : s.x0);
    }
    // of an entry whose key is a target (the sample is in range): dy = dbot : dtop, then the share of the tap's column
    template <int VEC> __device__ __forceinline__ void terms(int e, int ch, float *v) const
    {
        const int smp = e >> 2, tap = e & 3;
        const CropSample s = sample(smp);
        const float wy = tap & 2 ? s.ly : 1.0f - s.ly, wx = tap & 1 ? s.lx : 1.0f - s.lx;
        const float *row = grad_out + static_cast<long long>(smp) * c + ch;
        float g[VEC];
        if constexpr (VEC == 4) {
            const float4 q = *reinterpret_cast<const float4 *>(row);
            g[0] = q.x; g[1] = q.y; g[2] = q.z; g[3] = q.w;
        } else {
            g[0] = row[0];
        }
#pragma unroll
        for (int i = 0; i < VEC; ++i) v[i] = wx * (wy * g[i]);
    }
};

// 16-byte stores over the aligned body, dword stores over what is left in front of it and behind it
__global__ __launch_bounds__(256) void zero_fill_kernel(float *__restrict__ p, long long head, long long nvec, long long total)
{
    typedef float vec4 __attribute__((ext_vector_type(4)));
    const long long t = blockIdx.x * static_cast<long long>(blockDim.x) + threadIdx.x;
    const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
    vec4 *body = reinterpret_cast<vec4 *>(p + head);
    for (long long e = t; e < nvec; e += stride) body[e] = vec4{ 0.f, 0.f, 0.f, 0.f };
    const long long tail = head + nvec * 4;      // a few elements at most: the first threads take them
    if (t < head) p[t] = 0.0f;
    if (t < total - tail) p[tail + t] = 0.0f;
}

static int zero_fill(float *p, long long total, hipStream_t st)
{
    long long head = (16 - static_cast<long long>(reinterpret_cast<uintptr_t>(p) % 16)) % 16 / 4;   // floats up to a 16-byte boundary
    if (head > total) head = total;
    const long long nvec = (total - head) / 4;
    hipLaunchKernelGGL(zero_fill_kernel, dim3(grid_for(nvec, 256)), dim3(256), 0, st, p, head, nvec, total);
    return launch_status();
}

// a * b * c * d as element counts of fp32 tensors: false when the product, or its size in bytes, leaves long long
static bool elements(long long a, long long b, long long c, long long d, long long *out)
{
    long long p;
    if (__builtin_mul_overflow(a, b, &p) || __builtin_mul_overflow(p, c, &p) || __builtin_mul_overflow(p, d, &p)) return false;
    if (p > LLONG_MAX / 4) return false;
    *out = p;
    return true;
}

static int crop_args(int b, int h, int w, int c, long long n, int crop_h, int crop_w, long long *img_elems, long long *out_elems)
{
    if (b < 0 || n < 0 || h < 1 || w < 1 || c < 1 || crop_h < 1 || crop_w < 1) return HF_EINVAL;
    if (!elements(b, h, w, c, img_elems) || !elements(n, crop_h, crop_w, c, out_elems)) return HF_EINVAL;
    return HF_OK;
}

// b * h * w and n * crop_h * crop_w * 4 as ints, or false
static bool crop_grad_ordered_sizes(int b, int h, int w, int c, long long n, int crop_h, int crop_w, int *targets, int *entries)
{
    long long img_elems, out_elems, t, e;
    if (crop_args(b, h, w, c, n, crop_h, crop_w, &img_elems, &out_elems) != HF_OK) return false;
    if (!elements(b, h, w, 1, &t) || !elements(n, crop_h, crop_w, 4, &e) || t > INT_MAX || e > INT_MAX) return false;
    *targets = static_cast<int>(t);
    *entries = static_cast<int>(e);
    return true;
}

}  // namespace hf

using namespace hf;

HF_API int hf_roi_image_boxes(int b, int n, int h, int w, const float *boxes3d, const float *calib, float *box_px,
                              float *box_norm, float *box_yxyx, hf_stream_t stream)
{
    if (b < 0 || n < 0 || h < 1 || w < 1) return HF_EINVAL;
    const long long nbox = static_cast<long long>(b) * n;
    if (nbox > INT_MAX / kBoxLanes) return HF_EINVAL;      // the grid is one lane per corner
    if (nbox == 0) return HF_OK;
    if (!boxes3d || !calib) return HF_EINVAL;
    if (!box_px && !box_norm && !box_yxyx) return HF_OK;
    hipLaunchKernelGGL(roi_image_boxes_kernel, dim3(div_up(nbox * kBoxLanes, 256)), dim3(256), 0, as_stream(stream), n, nbox,
                       static_cast<float>(w), static_cast<float>(h), boxes3d, calib, box_px, box_norm, box_yxyx);
    return launch_status();
}

HF_API int hf_crop_and_resize(int b, int h, int w, int c, long long n, int crop_h, int crop_w, const float *img,
                              const float *boxes_yxyx, const int *box_ind, float extrapolation, float *out, hf_stream_t stream)
{
    long long img_elems, out_elems;
    if (crop_args(b, h, w, c, n, crop_h, crop_w, &img_elems, &out_elems) != HF_OK) return HF_EINVAL;
    if (n == 0 || b == 0) return HF_OK;
    if (!img || !boxes_yxyx || !box_ind || !out) return HF_EINVAL;
    const long long nsamples = n * crop_h * crop_w;
    const bool vec4 = c % 4 == 0 && (reinterpret_cast<uintptr_t>(img) | reinterpret_cast<uintptr_t>(out)) % 16 == 0;
    if (vec4)
        hipLaunchKernelGGL((crop_and_resize_kernel<4>), dim3(grid_for(nsamples * (c / 4), 256)), dim3(256), 0, as_stream(stream),
                           b, h, w, c, nsamples, crop_h, crop_w, img, boxes_yxyx, box_ind, extrapolation, out);
    else
        hipLaunchKernelGGL((crop_and_resize_kernel<1>), dim3(grid_for(out_elems, 256)), dim3(256), 0, as_stream(stream), b, h, w,
                           c, nsamples, crop_h, crop_w, img, boxes_yxyx, box_ind, extrapolation, out);
    return launch_status();
}

HF_API int hf_crop_and_resize_grad(int b, int h, int w, int c, long long n, int crop_h, int crop_w, const float *grad_out,
                                   const float *boxes_yxyx, const int *box_ind, float *grad_img, hf_stream_t stream)
{
    long long img_elems, out_elems;
    if (crop_args(b, h, w, c, n, crop_h, crop_w, &img_elems, &out_elems) != HF_OK) return HF_EINVAL;
    if (b > 0 && !grad_img) return HF_EINVAL;
    if (n > 0 && b > 0 && (!grad_out || !boxes_yxyx || !box_ind)) return HF_EINVAL;
    if (b == 0) return HF_OK;
    hipStream_t st = as_stream(stream);
    const int rc = zero_fill(grad_img, img_elems, st);
    if (rc != HF_OK) return rc;
    if (n == 0) return HF_OK;
    hipLaunchKernelGGL(crop_and_resize_grad_kernel, dim3(grid_for(out_elems, 256)), dim3(256), 0, st, b, h, w, c,
                       n * crop_h * crop_w, crop_h, crop_w, grad_out, boxes_yxyx, box_ind, grad_img);
    return launch_status();
}

HF_API size_t hf_crop_and_resize_grad_ordered_workspace(int b, int h, int w, int c, long long n, int crop_h, int crop_w)
{
    int targets, entries;
    if (!crop_grad_ordered_sizes(b, h, w, c, n, crop_h, crop_w, &targets, &entries) || targets == 0) return 0;
    return os_layout(targets, entries).total;
}

HF_API int hf_crop_and_resize_grad_ordered(int b, int h, int w, int c, long long n, int crop_h, int crop_w, const float *grad_out,
                                           const float *boxes_yxyx, const int *box_ind, float *grad_img, void *workspace,
                                           size_t workspace_bytes, hf_stream_t stream)
{
    int targets, entries;
    if (!crop_grad_ordered_sizes(b, h, w, c, n, crop_h, crop_w, &targets, &entries)) return HF_EINVAL;
    if (b == 0) return HF_OK;
    if (!grad_img || (entries > 0 && (!grad_out || !boxes_yxyx || !box_ind))) return HF_EINVAL;
    if (!workspace || reinterpret_cast<uintptr_t>(workspace) % 16 != 0 || workspace_bytes < os_layout(targets, entries).total)
        return HF_EINVAL;
    const CropGradEntries f = { b, h, w, c, crop_h, crop_w, grad_out, boxes_yxyx, box_ind };
    const bool vec4 = c % 4 == 0 && (reinterpret_cast<uintptr_t>(grad_out) | reinterpret_cast<uintptr_t>(grad_img)) % 16 == 0;
    return launch_ordered_scatter(f, targets, entries, c, vec4, grad_img, workspace, as_stream(stream));
}
