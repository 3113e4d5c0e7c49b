// conv_nhwc.hip -- the image pyramid's kernels for gfx950 (inference.ImgVggPyr, image_pyramid.py): 3x3 convolution, 3x3 stride-2
// transposed convolution and its adjoint, 2x2 max-pool, and for training the two weight gradients and the pool's gradient, on dense
// channel-last fp32 tensors, passed as rows of pixels.
//
//   conv3x3_kernel   A convolution in NHWC is the forward form of gemm_common.h, Z (R, N) = A (R, K) B^T (N, K), whose K axis is
//                    (tap, input channel) flattened: k = j cin + ci.  Row r of A is output pixel r, its element k is input pixel
//                    (oy + dy_j, ox + dx_j) of the same image at channel ci, zero when that pixel lies outside the image; row n of
//                    B is wt[tap_j][n][:].  The K axis is staged 32 wide whatever cin is, so the first layer (cin = 3, K = 27) is
//                    one stage and cin = 36 is eleven, not eighteen.  The MFMAs are fwd_mfma_stage's.  Loads of the next stage (or
//                    of the workgroup's next tile) are issued raw before the MFMAs of this one; what is out of range is replaced
//                    by zero when the stage is stored, from a mask kept in a register, so nothing waits on a load before the MFMAs.
//                    Epilogue: y = z scale + shift per output channel, max(., 0), into columns [y_col, y_col + cout) of rows
//                    y_stride wide.
//   UP               the transposed convolution (stride 2, padding 1, output_padding 1) is four such GEMMs, one per output parity
//                    class (py, px) = blockIdx.y: class pixels (qy, qx) are output pixels (2 qy + py, 2 qx + px), and only the
//                    (1 + py)(1 + px) taps that exist for the class are on the K axis: 1, 2, 2 and 4 taps, 9 in all for 4 pixels.
//   S2               the adjoint of UP, its input gradient: output pixel (oy, ox) gathers input pixels (2 oy - 1 + ky, 2 ox - 1 + kx).
//   maxpool2x2_kernel  one lane per output pixel and VEC channels, read from a column slice of wider rows.
//   conv_wgrad_kernel, maxpool2x2_bwd_kernel  the training direction, described where they stand.
// No kernel allocates, synchronises with the host or reads the environment.  Arithmetic: fp32, no contraction.
#include <limits.h>

#include "gemm_common.h"

namespace hf {

// tap j of the pass of parity class (py, px): the input pixel is (qy + dy, qx + dx), the weight matrix wt[wi]
// the three forms of conv3x3_kernel: the plain convolution, the transposed convolution (four parity passes), and the stride-2
// gather that is its adjoint (output pixel (oy, ox) reads input pixels (2 oy - 1 + ky, 2 ox - 1 + kx) of an image (2h, 2w))
constexpr int kConvPlain = 0, kConvUp = 1, kConvS2 = 2;

template <int MODE>
__device__ __forceinline__ void conv_tap(int j, int py, int px, int &dy, int &dx, int &wi)
{
    if constexpr (MODE != kConvUp) {
        const int ky = j / 3, kx = j - 3 * ky;
        dy = ky - 1; dx = kx - 1; wi = j;
    } else {
        // an even output row takes ky = 1 from iy = qy; an odd one ky = 0 from iy = qy + 1 and ky = 2 from iy = qy
        const int jy = px ? j >> 1 : j, jx = px ? j & 1 : 0;
        const int ky = py ? 2 * jy : 1, kx = px ? 2 * jx : 1;
        dy = py ? 1 - jy : 0; dx = px ? 1 - jx : 0; wi = 3 * ky + kx;
    }
}

constexpr int kRowOutside = INT_MIN / 2;  // qy of a staging row past the last pixel: every tap of it fails its range test

template <int NT, bool VEC, int MODE>
__global__ __launch_bounds__(kGemmThreads) __attribute__((amdgpu_waves_per_eu(2))) void conv3x3_kernel(
    int rows, int h, int w, int cin, int cout, int ntiles, const float *__restrict__ X, const float *__restrict__ in_sub,
    const float *__restrict__ W, const float *__restrict__ scale, const float *__restrict__ shift, int relu,
    float *__restrict__ Y, int y_stride, int y_col)
{
    __shared__ FwdLds<NT, 1> lds;

    constexpr bool UP = MODE == kConvUp, S2 = MODE == kConvS2;
    const int lane = threadIdx.x & 63;
    const int hin = S2 ? 2 * h : h, win = S2 ? 2 * w : w;      // the input image; h, w: the grid of pixels the rows run over
    const int py = UP ? blockIdx.y >> 1 : 0, px = UP ? blockIdx.y & 1 : 0;
    const int ntaps = UP ? (1 + py) * (1 + px) : 9;
    const int K = ntaps * cin, nstages = (K + kFwdKC - 1) / kFwdKC;
    const int k4 = fwd_k4(), srow = fwd_srow(), hw = h * w;

    int q[4], qy[4], qx[4];    // this thread's four staging rows of the tile: class pixel, its row and column in the image
    auto set_tile = [&](int tile) {
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const long long r = static_cast<long long>(tile) * kFwdRows + srow + 32 * p;
            const bool in = r < rows;
            const int rr = in ? static_cast<int>(r) : 0;
            const int rem = rr % hw;
            if constexpr (S2) {    // the input pixel (2 oy, 2 ox): 4 rows fits an int (launch_conv)
                const int oy = rem / w, ox = rem - oy * w;
                q[p] = 4 * (rr - rem) + 2 * oy * win + 2 * ox;
                qy[p] = in ? 2 * oy : kRowOutside;
                qx[p] = 2 * ox;
            } else {
                q[p] = rr;
                qy[p] = in ? rem / w : kRowOutside;
                qx[p] = rem % w;
            }
        }
    };

    float4 ar[4], br[NT], sub;
    unsigned amask, kmask;     // bit 4 p + e: element e of ar[p] is inside its image; bit e: k + e < K
    auto fetch = [&](int ks) {
        const int k = ks * kFwdKC + k4;
        amask = 0; kmask = 0;
        if constexpr (VEC) {
            const bool kin = k < K;
            const int j = kin ? k / cin : 0, ci = kin ? k - j * cin : 0;
            int dy, dx, wi;
            conv_tap<MODE>(j, py, px, dy, dx, wi);
            kmask = kin ? 0xfu : 0u;
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const bool ok = kin && static_cast<unsigned>(qy[p] + dy) < static_cast<unsigned>(hin) &&
                                static_cast<unsigned>(qx[p] + dx) < static_cast<unsigned>(win);
                const long long off = ok ? static_cast<long long>(q[p] + dy * win + dx) * cin + ci : 0;
                ar[p] = *reinterpret_cast<const float4 *>(X + off);
                amask |= ok ? 0xfu << (4 * p) : 0u;
            }
#pragma unroll
            for (int p = 0; p < NT; ++p) {
                const int n = srow + 32 * p;
                const long long off = (kin && n < cout) ? (static_cast<long long>(wi) * cout + n) * cin + ci : 0;
                br[p] = *reinterpret_cast<const float4 *>(W + off);
            }
            if (in_sub) sub = make_float4(in_sub[ci], in_sub[ci + 1], in_sub[ci + 2], in_sub[ci + 3]);
        } else {
            float a[4][4], b[NT][4], s[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const bool kin = k + e < K;
                const int j = kin ? (k + e) / cin : 0, ci = kin ? k + e - j * cin : 0;
                int dy, dx, wi;
                conv_tap<MODE>(j, py, px, dy, dx, wi);
                kmask |= kin ? 1u << e : 0u;
#pragma unroll
                for (int p = 0; p < 4; ++p) {
                    const bool ok = kin && static_cast<unsigned>(qy[p] + dy) < static_cast<unsigned>(hin) &&
                                    static_cast<unsigned>(qx[p] + dx) < static_cast<unsigned>(win);
                    a[p][e] = X[ok ? static_cast<long long>(q[p] + dy * win + dx) * cin + ci : 0];
                    amask |= ok ? 1u << (4 * p + e) : 0u;
                }
#pragma unroll
                for (int p = 0; p < NT; ++p) {
                    const int n = srow + 32 * p;
                    b[p][e] = W[(kin && n < cout) ? (static_cast<long long>(wi) * cout + n) * cin + ci : 0];
                }
                s[e] = in_sub ? in_sub[ci] : 0.f;
            }
#pragma unroll
            for (int p = 0; p < 4; ++p) ar[p] = make_float4(a[p][0], a[p][1], a[p][2], a[p][3]);
#pragma unroll
            for (int p = 0; p < NT; ++p) br[p] = make_float4(b[p][0], b[p][1], b[p][2], b[p][3]);
            sub = make_float4(s[0], s[1], s[2], s[3]);
        }
        if (!in_sub) sub = make_float4(0.f, 0.f, 0.f, 0.f);
    };

    if (static_cast<int>(blockIdx.x) < ntiles) {
        set_tile(blockIdx.x);
        fetch(0);
    }
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        f32x16 acc[NT];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int g = 0; g < 16; ++g) acc[nt][g] = 0.f;

        for (int ks = 0; ks < nstages; ++ks) {
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const unsigned m = amask >> (4 * p);
                float4 v;      // x - in_sub inside the image, zero in the padding and past K
                v.x = (m & 1u) ? ar[p].x - sub.x : 0.f;
                v.y = (m & 2u) ? ar[p].y - sub.y : 0.f;
                v.z = (m & 4u) ? ar[p].z - sub.z : 0.f;
                v.w = (m & 8u) ? ar[p].w - sub.w : 0.f;
                *reinterpret_cast<float4 *>(&lds.As[(srow + 32 * p) * kFwdLS + k4]) = v;
            }
#pragma unroll
            for (int p = 0; p < NT; ++p) {
                const bool nin = srow + 32 * p < cout;
                float4 v;
                v.x = (nin && (kmask & 1u)) ? br[p].x : 0.f;
                v.y = (nin && (kmask & 2u)) ? br[p].y : 0.f;
                v.z = (nin && (kmask & 4u)) ? br[p].z : 0.f;
                v.w = (nin && (kmask & 8u)) ? br[p].w : 0.f;
                *reinterpret_cast<float4 *>(&lds.Bs[(srow + 32 * p) * kFwdLS + k4]) = v;
            }
            __syncthreads();
            // the next stage -- of this tile, or the first one of the workgroup's next tile -- is in flight during the MFMAs
            // and the output stores below
            if (ks + 1 < nstages) {
                fetch(ks + 1);
            } else if (tile + static_cast<int>(gridDim.x) < ntiles) {
                set_tile(tile + gridDim.x);
                fetch(0);
            }
            fwd_mfma_stage(lds, acc);
            __syncthreads();
        }

        const long long row0 = static_cast<long long>(tile) * kFwdRows;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const int col = nt * 32 + (lane & 31);
            const bool col_in = col < cout;
            const float sc = (scale && col_in) ? scale[col] : 1.f, sh = (shift && col_in) ? shift[col] : 0.f;
#pragma unroll
            for (int g = 0; g < 16; ++g) {
                const long long r = fwd_d_row(row0, g);
                if (!col_in || r >= rows) continue;
                long long orow = r;
                if constexpr (UP) {
                    const int ri = static_cast<int>(r), img = ri / hw, rem = ri - img * hw, y = rem / w, x = rem - y * w;
                    orow = (static_cast<long long>(img) * (2 * h) + 2 * y + py) * (2 * w) + 2 * x + px;
                }
                float v = acc[nt][g] * sc + sh;
                if (relu) v = v < 0.f ? 0.f : v;
                Y[orow * y_stride + y_col + col] = v;
            }
        }
    }
}

template <int NT, bool VEC, int MODE>
static int launch_conv_nt(int rows, int h, int w, int cin, int cout, const float *x, const float *in_sub, const float *wt,
                          const float *scale, const float *shift, int relu, float *y, int y_stride, int y_col, hipStream_t st)
{
    const int ntiles = div_up(rows, kFwdRows);
    hipLaunchKernelGGL((conv3x3_kernel<NT, VEC, MODE>), dim3(resident_grid(NT, ntiles), MODE == kConvUp ? 4 : 1), dim3(kGemmThreads), 0, st, rows,
                       h, w, cin, cout, ntiles, x, in_sub, wt, scale, shift, relu, y, y_stride, y_col);
    return launch_status();
}

template <int MODE>
static int launch_conv(int b, int h, int w, int cin, int cout, const float *x, const float *in_sub, const float *wt,
                       const float *scale, const float *shift, int relu, float *y, int y_stride, int y_col, hipStream_t st)
{
    if (b < 1 || h < 1 || w < 1 || cin < 1 || cout < 1 || cout > 256 || y_col < 0 || y_stride - cout < y_col) return HF_EINVAL;
    if (!x || !wt || !y) return HF_EINVAL;
    const long long rows = static_cast<long long>(b) * h * w;
    if (rows > INT_MAX / (MODE == kConvPlain ? 1 : 4)) return HF_EINVAL;      // pixel rows are ints; element and byte offsets are 64-bit
    const int r = static_cast<int>(rows);
#define HF_CONV_NT(NT)                                                                                                           \
    return vec4_ok(x, cin) && vec4_ok(wt, cin)                                                                                   \
               ? launch_conv_nt<NT, true, MODE>(r, h, w, cin, cout, x, in_sub, wt, scale, shift, relu, y, y_stride, y_col, st)    \
               : launch_conv_nt<NT, false, MODE>(r, h, w, cin, cout, x, in_sub, wt, scale, shift, relu, y, y_stride, y_col, st)
    if (cout <= 32) { HF_CONV_NT(1); }
    if (cout <= 64) { HF_CONV_NT(2); }
    if (cout <= 128) { HF_CONV_NT(4); }
    HF_CONV_NT(8);
#undef HF_CONV_NT
}

// torch's max_pool2d: a NaN wins
__device__ __forceinline__ float pool_max(float m, float v) { return (v > m || v != v) ? v : m; }

template <int VEC>
__global__ __launch_bounds__(256) void maxpool2x2_kernel(long long total, int h, int w, int oh, int ow, int c,
                                                         const float *__restrict__ x, int x_stride, int x_col,
                                                         float *__restrict__ y)
{
    typedef float vec_t __attribute__((ext_vector_type(VEC)));
    const int cv = c / VEC;
    for (long long e = blockIdx.x * static_cast<long long>(blockDim.x) + threadIdx.x; e < total;
         e += static_cast<long long>(gridDim.x) * blockDim.x) {
        const long long pix = e / cv;
        const int l = static_cast<int>(e - pix * cv) * VEC;
        const long long t = pix / ow;
        const int ox = static_cast<int>(pix - t * ow);
        const long long img = t / oh;
        const int oy = static_cast<int>(t - img * oh);
        const float *p = x + ((img * h + 2 * oy) * w + 2 * ox) * x_stride + x_col + l;
        const vec_t v00 = *reinterpret_cast<const vec_t *>(p), v01 = *reinterpret_cast<const vec_t *>(p + x_stride);
        const vec_t v10 = *reinterpret_cast<const vec_t *>(p + static_cast<long long>(w) * x_stride);
        const vec_t v11 = *reinterpret_cast<const vec_t *>(p + (static_cast<long long>(w) + 1) * x_stride);
        vec_t m;
#pragma unroll
        for (int i = 0; i < VEC; ++i) m[i] = pool_max(pool_max(pool_max(v00[i], v01[i]), v10[i]), v11[i]);
        *reinterpret_cast<vec_t *>(y + pix * c + l) = m;
    }
}

// ------------------------------------------------------------------------------------------
// The weight gradients of both convolutions: one operand source for wgrad_tile_loop_staged.  dwt (9, cout, cin) is a (9 cout, cin)
// matrix, so the tap lies on the M axis of the wgrad form: column (t, co) of the G operand is channel co of dz at the pixel that tap t
// pairs with reduction row r, and the X operand is x' itself, unshifted.  A thread stages the same G columns for the whole kernel,
// so its tap is fixed and the shift is two constants per thread.
//   plain  rows run over the pixels p' of x: dwt[t][co][ci] = sum_p' dz[p' - tap_t][co] x'[p'][ci] (the forward's sum over output
//          pixels p with p' = p + tap_t); the padding of x never appears, a dz pixel outside the image is masked
//   UP     rows run over the input pixels (iy, ix): G is dz at (2 iy - 1 + ky, 2 ix - 1 + kx) of the (2h, 2w) image, masked where
//          that is negative (it never exceeds the image)
// Loads are raw; the mask is applied when the stage is stored.  Each of x and dz is read once per tile of the other axis.
// ------------------------------------------------------------------------------------------
template <int WN, bool GVEC, bool XVEC, bool UP>
__global__ __launch_bounds__(kGemmThreads) void conv_wgrad_kernel(int rows, int h, int w, int cin, int cout, int mtiles,
                                                                  long long rows_per_chunk, const float *__restrict__ X,
                                                                  const float *__restrict__ in_sub, const float *__restrict__ DZ,
                                                                  float *__restrict__ partial)
{
    using Q = WgradTile<2, WN>;
    __shared__ typename Q::Lds lds;
    const Q q(rows, mtiles, rows_per_chunk);
    const int M = 9 * cout, hw = h * w;
    constexpr int NE = GVEC ? 1 : 4;       // G elements of a float4 with a tap of their own

    int oy[NE], ox[NE], co[NE];            // the dz pixel of element e is (y + oy, x + ox) (UP: (2 y + oy, 2 x + ox)), its channel co
    bool cin_ok[NE];
#pragma unroll
    for (int e = 0; e < NE; ++e) {
        const int col = q.gcol + e;
        cin_ok[e] = col < M;
        const int t = cin_ok[e] ? col / cout : 0, ky = t / 3, kx = t - 3 * ky;
        co[e] = cin_ok[e] ? col - t * cout : 0;
        oy[e] = UP ? ky - 1 : 1 - ky;
        ox[e] = UP ? kx - 1 : 1 - kx;
    }
    float4 sub = make_float4(0.f, 0.f, 0.f, 0.f);
    if (in_sub) {
        sub.x = q.xcol < cin ? in_sub[q.xcol] : 0.f;
        sub.y = q.xcol + 1 < cin ? in_sub[q.xcol + 1] : 0.f;
        sub.z = q.xcol + 2 < cin ? in_sub[q.xcol + 2] : 0.f;
        sub.w = q.xcol + 3 < cin ? in_sub[q.xcol + 3] : 0.f;
    }

    float4 gr[Q::GPASS], xr[Q::XPASS];
    unsigned gmask;                        // bit 4 p + e: element e of gr[p] is a dz pixel inside its image
    auto fetch = [&](long long rt) {
        gmask = 0;
#pragma unroll
        for (int p = 0; p < Q::GPASS; ++p) {
            const long long r = rt + q.grow + p * Q::GROWS;
            const bool rin = r < q.r1;
            const int rr = rin ? static_cast<int>(r) : 0;
            const int img = rr / hw, rem = rr - img * hw, y = rem / w, x = rem - y * w;
            float g[NE];
            float4 g4;
#pragma unroll
            for (int e = 0; e < NE; ++e) {
                const int sy = (UP ? 2 * y : y) + oy[e], sx = (UP ? 2 * x : x) + ox[e];
                const bool ok = rin && cin_ok[e] && (UP ? (sy >= 0 && sx >= 0)
                                                        : (static_cast<unsigned>(sy) < static_cast<unsigned>(h) &&
                                                           static_cast<unsigned>(sx) < static_cast<unsigned>(w)));
                const int srow = UP ? 4 * (rr - rem) + sy * 2 * w + sx : rr - rem + sy * w + sx;
                const long long off = ok ? static_cast<long long>(srow) * cout + co[e] : 0;
                if constexpr (GVEC) {
                    g4 = *reinterpret_cast<const float4 *>(DZ + off);
                    gmask |= ok ? 0xfu << (4 * p) : 0u;
                } else {
                    g[e] = DZ[off];
                    gmask |= ok ? 1u << (4 * p + e) : 0u;
                }
            }
            if constexpr (GVEC) gr[p] = g4;
            else gr[p] = make_float4(g[0], g[NE > 1 ? 1 : 0], g[NE > 2 ? 2 : 0], g[NE > 3 ? 3 : 0]);
        }
#pragma unroll
        for (int p = 0; p < Q::XPASS; ++p) xr[p] = load4_guarded<XVEC>(X, rt + q.xrow + p * Q::XROWS, q.r1, q.xcol, cin);
    };
    auto stage_g = [&](int p) {
        const unsigned m = gmask >> (4 * p);
        float4 v;
        v.x = (m & 1u) ? gr[p].x : 0.f;
        v.y = (m & 2u) ? gr[p].y : 0.f;
        v.z = (m & 4u) ? gr[p].z : 0.f;
        v.w = (m & 8u) ? gr[p].w : 0.f;
        return v;
    };
    // x' = x - in_sub on the rows of the chunk; columns past cin hold zero minus zero
    auto stage_x = [&](int p, long long rt) {
        const bool rin = rt + q.xrow + p * Q::XROWS < q.r1;
        float4 v;
        v.x = rin ? xr[p].x - sub.x : 0.f;
        v.y = rin ? xr[p].y - sub.y : 0.f;
        v.z = rin ? xr[p].z - sub.z : 0.f;
        v.w = rin ? xr[p].w - sub.w : 0.f;
        return v;
    };
    wgrad_tile_loop_staged<2, WN>(lds, q, M, cin, partial, fetch, stage_g, stage_x);
}

// the plan of both weight gradients: wgrad_plan of the (9 cout, cin) matrix, always with the 128-row M tile
static WgradPlan conv_wgrad_plan(long long rows, int cin, int cout)
{
    WgradPlan p = wgrad_plan(rows, 9 * cout, cin);
    if (p.wm != 2) { p.wm = 2; p.mtiles = 1; }      // 9 cout <= 64: one tile, partly empty
    return p;
}

static bool conv_wgrad_contract(int b, int h, int w, int cin, int cout, bool up)
{
    if (b < 1 || h < 1 || w < 1 || cin < 1 || cout < 1 || cout > 256 || cin > 512) return false;
    return static_cast<long long>(b) * h * w <= INT_MAX / (up ? 4 : 1);
}

static size_t conv_wgrad_workspace(int b, int h, int w, int cin, int cout, bool up)
{
    if (!conv_wgrad_contract(b, h, w, cin, cout, up)) return 0;
    const WgradPlan p = conv_wgrad_plan(static_cast<long long>(b) * h * w, cin, cout);
    return p.chunks > 1 ? sizeof(float) * static_cast<size_t>(p.chunks) * 9 * cout * cin : 0;   // a single chunk writes dwt itself
}

template <bool UP>
static int launch_conv_wgrad(int b, int h, int w, int cin, int cout, const float *x, const float *in_sub, const float *dz, float *dwt,
                             void *workspace, size_t workspace_bytes, hipStream_t st)
{
    if (!conv_wgrad_contract(b, h, w, cin, cout, UP) || !x || !dz || !dwt) return HF_EINVAL;
    const int rows = b * h * w;
    const WgradPlan p = conv_wgrad_plan(rows, cin, cout);
    if (p.chunks > 65535) return HF_EINVAL;
    if (p.chunks > 1 && (!workspace || workspace_bytes < conv_wgrad_workspace(b, h, w, cin, cout, UP))) return HF_EINVAL;
    float *partial = p.chunks > 1 ? static_cast<float *>(workspace) : dwt;
    const dim3 grid(p.mtiles * p.ntiles, p.chunks);
    const bool gvec = vec4_ok(dz, cout), xvec = vec4_ok(x, cin);
#define HF_CWGRAD(WN, GV, XV)                                                                                                   \
    hipLaunchKernelGGL((conv_wgrad_kernel<WN, GV, XV, UP>), grid, dim3(kGemmThreads), 0, st, rows, h, w, cin, cout, p.mtiles,    \
                       p.rows_per_chunk, x, in_sub, dz, partial)
#define HF_CWGRAD_V(WN)                                                                                                         \
    do {                                                                                                                        \
        if (gvec && xvec) HF_CWGRAD(WN, true, true);                                                                            \
        else if (gvec) HF_CWGRAD(WN, true, false);                                                                              \
        else if (xvec) HF_CWGRAD(WN, false, true);                                                                              \
        else HF_CWGRAD(WN, false, false);                                                                                       \
    } while (0)
    if (p.wn == 2) HF_CWGRAD_V(2);
    else HF_CWGRAD_V(1);
#undef HF_CWGRAD_V
#undef HF_CWGRAD
    if (p.chunks > 1) launch_partial_reduce(9 * cout * cin, p.chunks, partial, dwt, st);      // chunks ascending: a fixed order
    return launch_status();
}

// The pool's gradient: one lane per 2x2 cell and VEC channels.  The argmax is recomputed from x with pool_max's rule (a strictly
// greater value or a NaN replaces the maximum, so the first maximum wins a tie), the index carried with it.  accumulate = 0 writes
// every pixel of the slice: the gradient at the argmax, zero elsewhere, zero in a last odd row or column; accumulate = 1 adds the same
// values to the pixels of whole windows and touches nothing else.
template <int VEC>
__global__ __launch_bounds__(256) void maxpool2x2_bwd_kernel(long long total, int h, int w, int ch, int cw, int c,
                                                             const float *__restrict__ x, int x_stride, int x_col,
                                                             const float *__restrict__ dpooled, float *__restrict__ dx,
                                                             int dx_stride, int dx_col, int accumulate)
{
    typedef float vec_t __attribute__((ext_vector_type(VEC)));
    const int cv = c / VEC, oh = h / 2, ow = w / 2;
    for (long long e = blockIdx.x * static_cast<long long>(blockDim.x) + threadIdx.x; e < total;
         e += static_cast<long long>(gridDim.x) * blockDim.x) {
        const long long cell = e / cv;
        const int l = static_cast<int>(e - cell * cv) * VEC;
        const long long t = cell / cw;
        const int cx = static_cast<int>(cell - t * cw);
        const long long img = t / ch;
        const int cy = static_cast<int>(t - img * ch);
        const bool y1 = 2 * cy + 1 < h, x1 = 2 * cx + 1 < w;
        const long long pix = (img * h + 2 * cy) * w + 2 * cx;
        float *d = dx + pix * dx_stride + dx_col + l;
        const long long down = static_cast<long long>(w) * dx_stride;
        if (y1 && x1) {
            const float *p = x + pix * x_stride + x_col + l;
            const vec_t v00 = *reinterpret_cast<const vec_t *>(p), v01 = *reinterpret_cast<const vec_t *>(p + x_stride);
            const vec_t v10 = *reinterpret_cast<const vec_t *>(p + static_cast<long long>(w) * x_stride);
            const vec_t v11 = *reinterpret_cast<const vec_t *>(p + (static_cast<long long>(w) + 1) * x_stride);
            const vec_t g = *reinterpret_cast<const vec_t *>(dpooled + ((img * oh + cy) * ow + cx) * c + l);
            vec_t o00, o01, o10, o11;
#pragma unroll
            for (int i = 0; i < VEC; ++i) {
                float m = v00[i];
                int k = 0;
                if (v01[i] > m || v01[i] != v01[i]) { m = v01[i]; k = 1; }
                if (v10[i] > m || v10[i] != v10[i]) { m = v10[i]; k = 2; }
                if (v11[i] > m || v11[i] != v11[i]) { m = v11[i]; k = 3; }
                o00[i] = k == 0 ? g[i] : 0.f; o01[i] = k == 1 ? g[i] : 0.f;
                o10[i] = k == 2 ? g[i] : 0.f; o11[i] = k == 3 ? g[i] : 0.f;
            }
            if (accumulate) {
                o00 += *reinterpret_cast<const vec_t *>(d); o01 += *reinterpret_cast<const vec_t *>(d + dx_stride);
                o10 += *reinterpret_cast<const vec_t *>(d + down); o11 += *reinterpret_cast<const vec_t *>(d + down + dx_stride);
            }
            *reinterpret_cast<vec_t *>(d) = o00; *reinterpret_cast<vec_t *>(d + dx_stride) = o01;
            *reinterpret_cast<vec_t *>(d + down) = o10; *reinterpret_cast<vec_t *>(d + down + dx_stride) = o11;
        } else if (!accumulate) {          // a cell of the dropped odd row or column: no window, no gradient
            vec_t zero;
#pragma unroll
            for (int i = 0; i < VEC; ++i) zero[i] = 0.f;
            *reinterpret_cast<vec_t *>(d) = zero;
            if (x1) *reinterpret_cast<vec_t *>(d + dx_stride) = zero;
            if (y1) *reinterpret_cast<vec_t *>(d + down) = zero;
        }
    }
}

}  // namespace hf

using namespace hf;

HF_API int hf_conv3x3_nhwc(int b, int h, int w, int cin, int cout, const float *x, const float *in_sub, const float *wt,
                           const float *scale, const float *shift, int relu, float *y, int y_stride, int y_col,
                           hf_stream_t stream)
{
    return launch_conv<kConvPlain>(b, h, w, cin, cout, x, in_sub, wt, scale, shift, relu, y, y_stride, y_col, as_stream(stream));
}

HF_API int hf_upconv3x3s2_nhwc(int b, int h, int w, int cin, int cout, const float *x, const float *wt, const float *scale,
                               const float *shift, int relu, float *y, int y_stride, int y_col, hf_stream_t stream)
{
    return launch_conv<kConvUp>(b, h, w, cin, cout, x, nullptr, wt, scale, shift, relu, y, y_stride, y_col, as_stream(stream));
}

HF_API int hf_maxpool2x2_nhwc(int b, int h, int w, int c, const float *x, int x_stride, int x_col, float *y, hf_stream_t stream)
{
    if (b < 1 || h < 1 || w < 1 || c < 1 || x_col < 0 || x_stride - c < x_col || !x || !y) return HF_EINVAL;
    const int oh = h / 2, ow = w / 2;
    const long long pixels = static_cast<long long>(b) * oh * ow;
    if (pixels == 0) return HF_OK;
    const bool vec4 = c % 4 == 0 && x_stride % 4 == 0 && x_col % 4 == 0 &&
                      (reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y)) % 16 == 0;
    if (vec4)
        hipLaunchKernelGGL((maxpool2x2_kernel<4>), dim3(grid_for(pixels * (c / 4), 256)), dim3(256), 0, as_stream(stream),
                           pixels * (c / 4), h, w, oh, ow, c, x, x_stride, x_col, y);
    else
        hipLaunchKernelGGL((maxpool2x2_kernel<1>), dim3(grid_for(pixels * c, 256)), dim3(256), 0, as_stream(stream), pixels * c, h,
                           w, oh, ow, c, x, x_stride, x_col, y);
    return launch_status();
}

HF_API int hf_conv3x3s2_nhwc(int b, int h, int w, int cin, int cout, const float *x, const float *wt, const float *scale,
                             const float *shift, int relu, float *y, int y_stride, int y_col, hf_stream_t stream)
{
    return launch_conv<kConvS2>(b, h, w, cin, cout, x, nullptr, wt, scale, shift, relu, y, y_stride, y_col, as_stream(stream));
}

HF_API size_t hf_conv3x3_nhwc_wgrad_workspace(int b, int h, int w, int cin, int cout)
{
    return conv_wgrad_workspace(b, h, w, cin, cout, false);
}

HF_API int hf_conv3x3_nhwc_wgrad(int b, int h, int w, int cin, int cout, const float *x, const float *in_sub, const float *dz,
                                 float *dwt, void *workspace, size_t workspace_bytes, hf_stream_t stream)
{
    return launch_conv_wgrad<false>(b, h, w, cin, cout, x, in_sub, dz, dwt, workspace, workspace_bytes, as_stream(stream));
}

HF_API size_t hf_upconv3x3s2_nhwc_wgrad_workspace(int b, int h, int w, int cin, int cout)
{
    return conv_wgrad_workspace(b, h, w, cin, cout, true);
}

HF_API int hf_upconv3x3s2_nhwc_wgrad(int b, int h, int w, int cin, int cout, const float *x, const float *dz, float *dwt,
                                     void *workspace, size_t workspace_bytes, hf_stream_t stream)
{
    return launch_conv_wgrad<true>(b, h, w, cin, cout, x, nullptr, dz, dwt, workspace, workspace_bytes, as_stream(stream));
}

HF_API int hf_maxpool2x2_nhwc_bwd(int b, int h, int w, int c, const float *x, int x_stride, int x_col, const float *dpooled, float *dx,
                                  int dx_stride, int dx_col, int accumulate, hf_stream_t stream)
{
    if (b < 1 || h < 1 || w < 1 || c < 1 || x_col < 0 || x_stride - c < x_col || dx_col < 0 || dx_stride - c < dx_col || !x || !dx)
        return HF_EINVAL;
    const bool windows = h > 1 && w > 1;
    if (windows && !dpooled) return HF_EINVAL;
    if (accumulate && !windows) return HF_OK;      // nothing to add
    const int ch = (h + 1) / 2, cw = (w + 1) / 2;
    const long long cells = static_cast<long long>(b) * ch * cw;
    const bool vec4 = c % 4 == 0 && x_stride % 4 == 0 && x_col % 4 == 0 && dx_stride % 4 == 0 && dx_col % 4 == 0 &&
                      (reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(dx) | reinterpret_cast<uintptr_t>(dpooled)) % 16 == 0;
    if (vec4)
        hipLaunchKernelGGL((maxpool2x2_bwd_kernel<4>), dim3(grid_for(cells * (c / 4), 256)), dim3(256), 0, as_stream(stream),
                           cells * (c / 4), h, w, ch, cw, c, x, x_stride, x_col, dpooled, dx, dx_stride, dx_col, accumulate);
    else
        hipLaunchKernelGGL((maxpool2x2_bwd_kernel<1>), dim3(grid_for(cells * c, 256)), dim3(256), 0, as_stream(stream), cells * c, h, w,
                           ch, cw, c, x, x_stride, x_col, dpooled, dx, dx_stride, dx_col, accumulate);
    return launch_status();
}
