// conv_nhwc_bf16.hip -- the image pyramid's inference convolutions on the bf16 matrix cores (hf_conv3x3_nhwc_bf16,
// hf_upconv3x3s2_nhwc_bf16): the semantics of conv3x3_kernel of conv_nhwc.hip (tap numbering, zero padding, in_sub inside the image
// only, the four parity classes of the up-convolution with their 1, 2, 2 and 4 taps, the two-step epilogue, the column slice) with
// bf16 operands.  Tensors stay fp32 in memory.
//
// Arithmetic.  Activation operand: bf16(fl32(x - in_sub)) inside the image, zero in the padding and past K -- one fp32 subtraction
// (no contraction), then the packed hardware conversion (pack_bf16x2, nearest even), between the global load and the LDS store.
// Weight operand: (9, cout, cin) bf16, converted once by hf_f32_to_bf16.  Accumulation fp32 (v_mfma_f32_16x16x32_bf16); epilogue
// fp32: y = z scale + shift rounded in two steps, max(., 0).
//
// K axis.  (tap, input channel) flattened, k = j cin + ci, staged 64 wide (two MFMA k-steps) whatever cin is: the first layer
// (cin = 3, K = 27) is one stage, cin = 36 is ceil(324 / 64) = 6 stages.  A last stage with at most 32 channels left issues one
// k-step, not two: K = 27 runs a single MFMA k-step.
//
// Tile machine (linear_bf16.hip's).  A workgroup of 2 x WN waves owns 128 pixel rows and all cout <= 16 NT WN columns; a wave owns
// 64 rows x 16 NT columns as NT x 4 accumulator tiles.  The MFMA's A operand is the weight tile and its B operand the pixel tile, so
// a lane holds four CONSECUTIVE output columns of one pixel and stores them sixteen bytes at a time where y, y_col, y_stride and cout
// allow (all multiples of four floats), as four scalars elsewhere.
// Dispatch (launch_conv_bf16): the column tile is the smallest of 32, 64, 128, 256 that holds cout -- the pyramid's four widths --
//   cout <= 32: <NT 1, WN 2>   cout <= 64: <2, 2>   cout <= 128: <4, 2>   beyond: <4, 4> (eight waves)
// so no layer runs MFMAs on more than the columns past its own width rounded up to the tile; times VEC (cin % 4 == 0, x 16-byte and
// wt_bf16 8-byte aligned: a staged quad lies inside one tap; otherwise every element has its own tap and is loaded alone) times the
// plain / up-convolution form: sixteen kernels.  One workgroup per 128-row tile (times four parity classes, blockIdx.y, for UP).
//
// LDS.  A 64-wide stage of both operands as bf16 with k contiguous, row stride 80 bf16 = 10 sixteen-byte slots: the derivation in
// linear_bf16.hip's header (ds_read_b128 in groups of 16 lanes, any stride of 2 mod 4 slots is conflict-free) applies unchanged,
// the fragments are read the same way.  At most 20 + 40 KB per workgroup: two workgroups per CU fit.
//
// Prefetch.  The next stage's global loads are issued raw before the current stage's MFMAs; the padding / past-K mask is kept in a
// register and applied when the stage is stored, so nothing waits on a load before the MFMAs.  Which taps exist for a staged pixel
// depends on the pixel alone: a nine-bit mask per staging row, formed once.
// Every form is held to 256 VGPRs (amdgpu_waves_per_eu(2)): no spills, no scratch (profiles/conv_nhwc_bf16_instantiations.md).
// No kernel allocates, synchronises with the host or reads the environment; the summation order is fixed: two calls, the same bits.
#include <limits.h>

#include "bf16_common.h"
#include "gemm_common.h"
#include "hf_common.h"

namespace hf {

constexpr int kCbRows = 128;          // pixel rows per workgroup tile
constexpr int kCbKC = 64;             // K elements per LDS stage: two MFMA k-steps
constexpr int kCbLS = kCbKC + 16;     // LDS row stride in bf16 elements (linear_bf16.hip's kBfLS)

// tap j of the pass of parity class (py, px), as conv_tap of conv_nhwc.hip: the input pixel is (qy + dy, qx + dx), the weight
// matrix wt[wi]
template <bool UP>
__device__ __forceinline__ void conv_bf16_tap(int j, int py, int px, int &dy, int &dx, int &wi)
{
    if constexpr (!UP) {
        const int ky = j / 3, kx = j - 3 * ky;
        dy = ky - 1; dx = kx - 1; wi = j;
    } else {
        // an even output row takes ky = 1 from iy = qy; an odd one ky = 0 from iy = qy + 1 and ky = 2 from iy = qy
        const int jy = px ? j >> 1 : j, jx = px ? j & 1 : 0;
        const int ky = py ? 2 * jy : 1, kx = px ? 2 * jx : 1;
        dy = py ? 1 - jy : 0; dx = px ? 1 - jx : 0; wi = 3 * ky + kx;
    }
}

template <int NT, int WN>
struct alignas(16) ConvBfLds {
    uint16_t Xs[kCbRows * kCbLS];
    uint16_t Ws[16 * NT * WN * kCbLS];
};

template <int NT, int WN, bool VEC, bool UP>
__global__ __launch_bounds__(128 * WN) __attribute__((amdgpu_waves_per_eu(2))) void conv3x3_bf16_kernel(
    int rows, int h, int w, int cin, int cout, const float *__restrict__ X, const float *__restrict__ in_sub,
    const uint16_t *__restrict__ W, const float *__restrict__ scale, const float *__restrict__ shift, int relu,
    float *__restrict__ Y, int y_stride, int y_col, int vec_store)
{
    constexpr int THREADS = 128 * WN, BN = 16 * NT * WN;
    constexpr int SROWS = THREADS / 16;           // rows staged per pass: 16 threads cover the 64 k of a row, 4 each
    constexpr int XP = kCbRows / SROWS, WP = BN / SROWS;
    static_assert(XP <= 8 && WP >= 1, "the staging masks hold four bits for each of at most eight rows");
    __shared__ ConvBfLds<NT, WN> lds;

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int wm = wave & 1, wn = wave >> 1;
    const int kq = (t & 15) * 4, srow = t >> 4;
    const int py = UP ? blockIdx.y >> 1 : 0, px = UP ? blockIdx.y & 1 : 0;
    const int ntaps = UP ? (1 + py) * (1 + px) : 9;
    const int K = ntaps * cin, hw = h * w;
    const long long row0 = static_cast<long long>(blockIdx.x) * kCbRows;

    // this thread's XP staging rows: the pixel's row index, and bit j of taps[p]: tap j of the class reads a pixel of the image
    int q[XP];
    unsigned taps[XP];
#pragma unroll
    for (int p = 0; p < XP; ++p) {
        const long long r = row0 + srow + p * SROWS;
        const bool in = r < rows;
        q[p] = in ? static_cast<int>(r) : 0;
        const int rem = q[p] % hw, qy = rem / w, qx = rem - qy * w;
        unsigned m = 0;
#pragma unroll
        for (int j = 0; j < (UP ? 4 : 9); ++j) {
            int dy, dx, wi;
            conv_bf16_tap<UP>(j, py, px, dy, dx, wi);
            const bool ok = in && j < ntaps && static_cast<unsigned>(qy + dy) < static_cast<unsigned>(h) &&
                            static_cast<unsigned>(qx + dx) < static_cast<unsigned>(w);
            m |= ok ? 1u << j : 0u;
        }
        taps[p] = m;
    }

    float4 xr[XP], sub;
    uint2 wr[WP];
    unsigned amask, kmask;     // bit 4 p + e: element e of xr[p] is inside its image and k + e < K; bit e: k + e < K
    auto fetch = [&](int k0) {
        const int k = k0 + kq;
        amask = 0; kmask = 0;
        if constexpr (VEC) {
            const bool kin = k < K;
            const int j = kin ? k / cin : 0, ci = kin ? k - j * cin : 0;
            int dy, dx, wi;
            conv_bf16_tap<UP>(j, py, px, dy, dx, wi);
            kmask = kin ? 0xfu : 0u;
            const int doff = dy * w + dx;
#pragma unroll
            for (int p = 0; p < XP; ++p) {
                const bool ok = kin && ((taps[p] >> j) & 1u);
                const long long off = ok ? static_cast<long long>(q[p] + doff) * cin + ci : 0;
                xr[p] = *reinterpret_cast<const float4 *>(X + off);
                amask |= ok ? 0xfu << (4 * p) : 0u;
            }
#pragma unroll
            for (int p = 0; p < WP; ++p) {
                const int n = srow + p * SROWS;
                const long long off = (kin && n < cout) ? (static_cast<long long>(wi) * cout + n) * cin + ci : 0;
                wr[p] = *reinterpret_cast<const uint2 *>(W + off);
            }
            sub = in_sub ? make_float4(in_sub[ci], in_sub[ci + 1], in_sub[ci + 2], in_sub[ci + 3]) : make_float4(0.f, 0.f, 0.f, 0.f);
        } else {
            float a[XP][4], s[4];
            unsigned b[WP][4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const bool kin = k + e < K;
                const int j = kin ? (k + e) / cin : 0, ci = kin ? k + e - j * cin : 0;
                int dy, dx, wi;
                conv_bf16_tap<UP>(j, py, px, dy, dx, wi);
                kmask |= kin ? 1u << e : 0u;
                const int doff = dy * w + dx;
#pragma unroll
                for (int p = 0; p < XP; ++p) {
                    const bool ok = kin && ((taps[p] >> j) & 1u);
                    a[p][e] = X[ok ? static_cast<long long>(q[p] + doff) * cin + ci : 0];
                    amask |= ok ? 1u << (4 * p + e) : 0u;
                }
#pragma unroll
                for (int p = 0; p < WP; ++p) {
                    const int n = srow + p * SROWS;
                    b[p][e] = W[(kin && n < cout) ? (static_cast<long long>(wi) * cout + n) * cin + ci : 0];
                }
                s[e] = in_sub ? in_sub[ci] : 0.f;
            }
#pragma unroll
            for (int p = 0; p < XP; ++p) xr[p] = make_float4(a[p][0], a[p][1], a[p][2], a[p][3]);
#pragma unroll
            for (int p = 0; p < WP; ++p) wr[p] = make_uint2(b[p][0] | (b[p][1] << 16), b[p][2] | (b[p][3] << 16));
            sub = make_float4(s[0], s[1], s[2], s[3]);
        }
    };

    f32x4 acc[NT][4];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) acc[nt][mt] = f32x4{ 0.f, 0.f, 0.f, 0.f };

    const bool wave_has_columns = wn * 16 * NT < cout;  // a wave wholly past cout stages and synchronises only
    const uint16_t *xf = lds.Xs + (wm * 64 + (lane & 15)) * kCbLS + (lane >> 4) * 8;
    const uint16_t *wf = lds.Ws + (wn * 16 * NT + (lane & 15)) * kCbLS + (lane >> 4) * 8;

    fetch(0);
    for (int k0 = 0; k0 < K; k0 += kCbKC) {
#pragma unroll
        for (int p = 0; p < XP; ++p) {
            const unsigned m = amask >> (4 * p);
            // x - in_sub inside the image, zero in the padding and past K; then the packed conversion
            const float v0 = (m & 1u) ? xr[p].x - sub.x : 0.f, v1 = (m & 2u) ? xr[p].y - sub.y : 0.f;
            const float v2 = (m & 4u) ? xr[p].z - sub.z : 0.f, v3 = (m & 8u) ? xr[p].w - sub.w : 0.f;
            *reinterpret_cast<uint2 *>(&lds.Xs[(srow + p * SROWS) * kCbLS + kq]) = make_uint2(pack_bf16x2(v0, v1), pack_bf16x2(v2, v3));
        }
#pragma unroll
        for (int p = 0; p < WP; ++p) {
            const bool nin = srow + p * SROWS < cout;
            const unsigned lo = ((nin && (kmask & 1u)) ? 0x0000ffffu : 0u) | ((nin && (kmask & 2u)) ? 0xffff0000u : 0u);
            const unsigned hi = ((nin && (kmask & 4u)) ? 0x0000ffffu : 0u) | ((nin && (kmask & 8u)) ? 0xffff0000u : 0u);
            *reinterpret_cast<uint2 *>(&lds.Ws[(srow + p * SROWS) * kCbLS + kq]) = make_uint2(wr[p].x & lo, wr[p].y & hi);
        }
        __syncthreads();
        if (k0 + kCbKC < K) fetch(k0 + kCbKC);    // in flight during the MFMAs below
        if (wave_has_columns) {
            const int ksteps = K - k0 > 32 ? 2 : 1;    // a last stage of at most 32 channels: no second, empty k-step
#pragma unroll
            for (int ks = 0; ks < kCbKC / 32; ++ks) {
                if (ks < ksteps) {
                    bf16x8 a[NT], b[4];
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt) a[nt] = *reinterpret_cast<const bf16x8 *>(wf + nt * 16 * kCbLS + ks * 32);
#pragma unroll
                    for (int mt = 0; mt < 4; ++mt) b[mt] = *reinterpret_cast<const bf16x8 *>(xf + mt * 16 * kCbLS + ks * 32);
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                        for (int mt = 0; mt < 4; ++mt)
                            acc[nt][mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[nt], b[mt], acc[nt][mt], 0, 0, 0);
                }
            }
        }
        __syncthreads();
    }

    // epilogue: this lane holds columns n .. n + 3 of pixel row `r` in acc[nt][mt]
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const int n = wn * 16 * NT + nt * 16 + (lane >> 4) * 4;
        if (n >= cout) continue;
        float sc[4], sh[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const bool col_in = n + i < cout;
            sc[i] = (scale && col_in) ? scale[n + i] : 1.f;
            sh[i] = (shift && col_in) ? shift[n + i] : 0.f;
        }
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
            const long long r = row0 + wm * 64 + mt * 16 + (lane & 15);
            if (r >= rows) continue;
            long long orow = r;
            if constexpr (UP) {
                const int ri = static_cast<int>(r), img = ri / hw, rem = ri - img * hw, y = rem / w, x = rem - y * w;
                orow = (static_cast<long long>(img) * (2 * h) + 2 * y + py) * (2 * w) + 2 * x + px;
            }
            float o[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                float v = acc[nt][mt][i] * sc[i] + sh[i];
                if (relu) v = v < 0.f ? 0.f : v;
                o[i] = v;
            }
            float *dst = Y + orow * y_stride + y_col + n;
            if (vec_store) {
                *reinterpret_cast<float4 *>(dst) = make_float4(o[0], o[1], o[2], o[3]);
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (n + i < cout) dst[i] = o[i];
            }
        }
    }
}

template <int NT, int WN, bool UP>
static int launch_conv_bf16_tile(int rows, int h, int w, int cin, int cout, const float *x, const float *in_sub, const uint16_t *wt,
                                 const float *scale, const float *shift, int relu, float *y, int y_stride, int y_col, hipStream_t st)
{
    const dim3 grid(div_up(rows, kCbRows), UP ? 4 : 1);
    const bool vec = cin % 4 == 0 && bf_aligned16(x) && reinterpret_cast<uintptr_t>(wt) % 8 == 0;
    const int vec_store = cout % 4 == 0 && y_stride % 4 == 0 && y_col % 4 == 0 && bf_aligned16(y);
    if (vec)
        hipLaunchKernelGGL((conv3x3_bf16_kernel<NT, WN, true, UP>), grid, dim3(128 * WN), 0, st, rows, h, w, cin, cout, x, in_sub, wt, scale,
                           shift, relu, y, y_stride, y_col, vec_store);
    else
        hipLaunchKernelGGL((conv3x3_bf16_kernel<NT, WN, false, UP>), grid, dim3(128 * WN), 0, st, rows, h, w, cin, cout, x, in_sub, wt, scale,
                           shift, relu, y, y_stride, y_col, vec_store);
    return launch_status();
}

template <bool UP>
static int launch_conv_bf16(int b, int h, int w, int cin, int cout, const float *x, const float *in_sub, const uint16_t *wt,
                            const float *scale, const float *shift, int relu, float *y, int y_stride, int y_col, hipStream_t st)
{
    if (b < 1 || h < 1 || w < 1 || cin < 1 || cout < 1 || cout > 256 || y_col < 0 || y_stride - cout < y_col) return HF_EINVAL;
    if (!x || !wt || !y) return HF_EINVAL;
    const long long rows = static_cast<long long>(b) * h * w;
    if (rows > INT_MAX / (UP ? 4 : 1)) return HF_EINVAL;      // pixel rows are ints; element and byte offsets are 64-bit
    const int r = static_cast<int>(rows);
#define HF_CONV_BF16(NT, WN) \
    return launch_conv_bf16_tile<NT, WN, UP>(r, h, w, cin, cout, x, in_sub, wt, scale, shift, relu, y, y_stride, y_col, st)
    if (cout <= 32) { HF_CONV_BF16(1, 2); }
    if (cout <= 64) { HF_CONV_BF16(2, 2); }
    if (cout <= 128) { HF_CONV_BF16(4, 2); }
    HF_CONV_BF16(4, 4);
#undef HF_CONV_BF16
}

}  // namespace hf

using namespace hf;

HF_API int hf_conv3x3_nhwc_bf16(int b, int h, int w, int cin, int cout, const float *x, const float *in_sub, const uint16_t *wt_bf16,
                                const float *scale, const float *shift, int relu, float *y, int y_stride, int y_col,
                                hf_stream_t stream)
{
    return launch_conv_bf16<false>(b, h, w, cin, cout, x, in_sub, wt_bf16, scale, shift, relu, y, y_stride, y_col, as_stream(stream));
}

HF_API int hf_upconv3x3s2_nhwc_bf16(int b, int h, int w, int cin, int cout, const float *x, const uint16_t *wt_bf16, const float *scale,
                                    const float *shift, int relu, float *y, int y_stride, int y_col, hf_stream_t stream)
{
    return launch_conv_bf16<true>(b, h, w, cin, cout, x, nullptr, wt_bf16, scale, shift, relu, y, y_stride, y_col, as_stream(stream));
}
