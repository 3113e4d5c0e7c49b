// linear_bf16.hip -- inference-only dense layers on the bf16 matrix cores (hf_f32_to_bf16, hf_linear_bf16_fwd_eval).
//
// y (rows, cout) = epilogue( bf16(x) (rows, cin) . w_bf16^T (cout, cin) ), fp32 accumulation.  x stays fp32 in memory and is rounded
// to bf16 (nearest even, the packed hardware conversion) between its global load and the LDS store; the weight arrives converted.
// The epilogue is the pass that otherwise follows the GEMM: + bias, the streaming ELU, the eval-mode BatchNorm affine, ReLU.
//
// Tile machine.  A workgroup of 2 x WN waves owns 128 rows x 16 NT WN columns; a wave owns 64 rows x 16 NT columns as NT x 4
// accumulator tiles of v_mfma_f32_16x16x32_bf16.  The MFMA's A operand is the WEIGHT tile and its B operand the x tile, so that D
// holds, per lane, one row of y and four CONSECUTIVE columns (D row = 4 (lane >> 4) + reg -> column, D column = lane & 15 -> row):
// the epilogue reads its per-column constants and stores y sixteen bytes at a time.
// LDS holds a 64-channel stage of both operands as bf16 with k contiguous; a lane's 8-element fragment (row lane & 15, channels
// 8 (lane >> 4) .. +7 of a 32-channel k-step) is one ds_read_b128.  The row stride is 80 bf16 = 160 bytes = 10 sixteen-byte slots:
// ds_read_b128 is served in four groups of 16 lanes, each made of 8 rows r (r mod 16 in 12 .. 15, 0 .. 3) of one slot column and the
// 8 other rows of the next; with a stride of s slots the group touches slots s r (first set) and s r + 1 (second set) mod 16, and
// s = 10 (any s = 2 mod 4) sends the first set to the eight even and the second to the eight odd slots: conflict-free.
// The next stage's global loads are issued before the current stage's MFMAs and waited for when the stage is stored.
// x is re-read once per column tile: the workgroups are renumbered so that consecutive tiles (the column tiles of one row block are
// consecutive) run on the same XCD at the same time and the re-reads hit its L2.  Wide layers take 256-column tiles on eight waves
// (two re-reads of x at 512 outputs).  Every form is held to 256 VGPRs (amdgpu_waves_per_eu(2)): no spills, no scratch.
// Measured (scripts/probes/bf16_linear_timing.py, profiles/bf16_inference_timing.json): 409600 x 2688 x 512 with the BatchNorm
// epilogue in 2.1 ms (525-540 TFLOP/s) against 7.9 ms for the fp32 library GEMM plus its BatchNorm pass and 2.55 ms for the library's
// bf16 GEMM with its cast and BatchNorm passes.  One workgroup walks all of cin for its tile: a short, deep product (800 x 11808)
// launches seven workgroups and loses to the library; mlp.bf16_route_pays keeps such shapes away.
#include "bf16_common.h"
#include "gemm_common.h"
#include "hf_common.h"

namespace hf {

constexpr int kBfRows = 128;          // rows per workgroup tile
constexpr int kBfKC = 64;             // channels per LDS stage: two MFMA k-steps
constexpr int kBfLS = kBfKC + 16;     // LDS row stride in bf16 elements (see above)
constexpr int kBfRelu = 1, kBfElu = 2;  // `mode`, the bits of the BatchNorm entry points' `relu`

// n floats; `vec`: src 16-byte and dst 8-byte aligned, whole quads take one 16-byte load and one 8-byte store
__global__ __launch_bounds__(256) void f32_to_bf16_kernel(long long n, int vec, const float *__restrict__ src, uint16_t *__restrict__ dst)
{
    const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
    const long long t = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
    const long long quads = vec ? n / 4 : 0;
    for (long long q = t; q < quads; q += stride) {
        const float4 v = *reinterpret_cast<const float4 *>(src + 4 * q);
        *reinterpret_cast<uint2 *>(dst + 4 * q) = make_uint2(pack_bf16x2(v.x, v.y), pack_bf16x2(v.z, v.w));
    }
    for (long long i = 4 * quads + t; i < n; i += stride) dst[i] = static_cast<uint16_t>(pack_bf16x2(src[i], 0.0f) & 0xffffu);
}

template <int NT, int WN>
struct alignas(16) BfLds {
    uint16_t Xs[kBfRows * kBfLS];
    uint16_t Ws[16 * NT * WN * kBfLS];
};

template <int NT, int WN>
__global__ __launch_bounds__(128 * WN) __attribute__((amdgpu_waves_per_eu(2))) void linear_bf16_kernel(long long rows, int cin, int cout, int col_tiles, const float *__restrict__ x,
                                                                const uint16_t *__restrict__ w, const float *__restrict__ bias,
                                                                const float *__restrict__ gamma, const float *__restrict__ beta,
                                                                const float *__restrict__ mean, const float *__restrict__ invstd, int mode,
                                                                float *__restrict__ y)
{
    constexpr int THREADS = 128 * WN, BN = 16 * NT * WN;
    constexpr int SROWS = THREADS / 16;           // rows staged per pass: 16 threads cover the 64 channels of a row, 4 each
    constexpr int XP = kBfRows / SROWS, WP = BN / SROWS;
    __shared__ BfLds<NT, WN> lds;

    // consecutive tiles on one XCD: workgroup b runs on XCD b % 8; the tail past a multiple of 8 keeps its number
    const unsigned per_xcd = gridDim.x / kNumXCD;
    const unsigned tile = blockIdx.x < per_xcd * kNumXCD ? (blockIdx.x % kNumXCD) * per_xcd + blockIdx.x / kNumXCD : blockIdx.x;
    const long long row0 = static_cast<long long>(tile / col_tiles) * kBfRows;
    const int n0 = static_cast<int>(tile % col_tiles) * BN;

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int wm = wave & 1, wn = wave >> 1;
    const int kq = (t & 15) * 4, srow = t >> 4;

    float4 xr[XP];
    uint2 wr[WP];
    // the loads of the stage at channel k0: zero outside the matrices (cin % 4 == 0: a quad is inside or outside as a whole)
    auto fetch = [&](int k0) {
        const int k = k0 + kq;
#pragma unroll
        for (int p = 0; p < XP; ++p) xr[p] = load4_guarded<true>(x, row0 + srow + p * SROWS, rows, k, cin);
#pragma unroll
        for (int p = 0; p < WP; ++p) {
            const int n = n0 + srow + p * SROWS;
            const bool ok = n < cout && k < cin;
            const uint2 v = *reinterpret_cast<const uint2 *>(w + (ok ? static_cast<size_t>(n) * cin + k : 0));
            wr[p] = ok ? v : make_uint2(0u, 0u);
        }
    };

    f32x4 acc[NT][4];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) acc[nt][mt] = f32x4{ 0.f, 0.f, 0.f, 0.f };

    const bool wave_has_columns = n0 + wn * 16 * NT < cout;  // a wave wholly past cout stages and synchronises only
    const uint16_t *xf = lds.Xs + (wm * 64 + (lane & 15)) * kBfLS + (lane >> 4) * 8;
    const uint16_t *wf = lds.Ws + (wn * 16 * NT + (lane & 15)) * kBfLS + (lane >> 4) * 8;

    fetch(0);
    for (int k0 = 0; k0 < cin; k0 += kBfKC) {
#pragma unroll
        for (int p = 0; p < XP; ++p)
            *reinterpret_cast<uint2 *>(&lds.Xs[(srow + p * SROWS) * kBfLS + kq]) =
                make_uint2(pack_bf16x2(xr[p].x, xr[p].y), pack_bf16x2(xr[p].z, xr[p].w));
#pragma unroll
        for (int p = 0; p < WP; ++p) *reinterpret_cast<uint2 *>(&lds.Ws[(srow + p * SROWS) * kBfLS + kq]) = wr[p];
        __syncthreads();
        if (k0 + kBfKC < cin) fetch(k0 + kBfKC);  // in flight during the MFMAs below
        if (wave_has_columns) {
#pragma unroll
            for (int ks = 0; ks < kBfKC / 32; ++ks) {
                bf16x8 a[NT], b[4];
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) a[nt] = *reinterpret_cast<const bf16x8 *>(wf + nt * 16 * kBfLS + ks * 32);
#pragma unroll
                for (int mt = 0; mt < 4; ++mt) b[mt] = *reinterpret_cast<const bf16x8 *>(xf + mt * 16 * kBfLS + ks * 32);
#pragma unroll
                for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                    for (int mt = 0; mt < 4; ++mt)
                        acc[nt][mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[nt], b[mt], acc[nt][mt], 0, 0, 0);
            }
        }
        __syncthreads();
    }

    // epilogue: this lane holds columns n .. n + 3 of row `row` in acc[nt][mt]
    const bool bn = gamma != nullptr;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const int n = n0 + wn * 16 * NT + nt * 16 + (lane >> 4) * 4;
        if (n >= cout) continue;  // cout % 4 == 0: the four columns are inside or outside together
        float a[4] = { 1.f, 1.f, 1.f, 1.f }, mu[4] = { 0.f, 0.f, 0.f, 0.f }, be[4] = { 0.f, 0.f, 0.f, 0.f }, bb[4] = { 0.f, 0.f, 0.f, 0.f };
        if (bias) {
#pragma unroll
            for (int i = 0; i < 4; ++i) bb[i] = bias[n + i];
        }
        if (bn) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                a[i] = gamma[n + i] * invstd[n + i];
                mu[i] = mean[n + i];
                be[i] = beta[n + i];
            }
        }
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
            const long long row = row0 + wm * 64 + mt * 16 + (lane & 15);
            if (row >= rows) continue;
            float o[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                float z = acc[nt][mt][i] + bb[i];
                if (bn) {  // y = a (x - mu) + beta: the difference first, as bn_apply_kernel of mlp.hip forms it
                    if (mode & kBfElu) z = elu_stream(z);
                    z = a[i] * (z - mu[i]) + be[i];
                    if (mode & kBfRelu) z = fmaxf(z, 0.0f);
                }
                o[i] = z;
            }
            *reinterpret_cast<float4 *>(y + row * cout + n) = make_float4(o[0], o[1], o[2], o[3]);
        }
    }
}

template <int NT, int WN>
static int launch_linear_bf16(long long rows, int cin, int cout, const float *x, const uint16_t *w, const float *bias, const float *gamma,
                              const float *beta, const float *mean, const float *invstd, int mode, float *y, hipStream_t st)
{
    const long long row_blocks = (rows + kBfRows - 1) / kBfRows;
    const int col_tiles = div_up(cout, 16 * NT * WN);
    if (row_blocks * col_tiles > 0x7fffffffLL) return HF_EINVAL;
    hipLaunchKernelGGL((linear_bf16_kernel<NT, WN>), dim3(static_cast<unsigned>(row_blocks * col_tiles)), dim3(128 * WN), 0, st, rows, cin,
                       cout, col_tiles, x, w, bias, gamma, beta, mean, invstd, mode, y);
    return launch_status();
}

}  // namespace hf

using namespace hf;

HF_API int hf_f32_to_bf16(long long n, const float *src, uint16_t *dst, hf_stream_t stream)
{
    if (n < 1 || !src || !dst) return HF_EINVAL;
    if (reinterpret_cast<uintptr_t>(src) % 4 != 0 || reinterpret_cast<uintptr_t>(dst) % 2 != 0) return HF_EINVAL;
    const int vec = bf_aligned16(src) && reinterpret_cast<uintptr_t>(dst) % 8 == 0;
    long long blocks = (n / 4 + 255) / 256;
    if (blocks < 1) blocks = 1;
    if (blocks > 8 * kNumCU) blocks = 8 * kNumCU;
    hipLaunchKernelGGL(f32_to_bf16_kernel, dim3(static_cast<unsigned>(blocks)), dim3(256), 0, as_stream(stream), n, vec, src, dst);
    return launch_status();
}

HF_API int hf_linear_bf16_fwd_eval(long long rows, int cin, int cout, const float *x, const uint16_t *w_bf16, const float *bias,
                                   const float *gamma, const float *beta, const float *mean, const float *invstd, int mode,
                                   float *y, hf_stream_t stream)
{
    if (rows < 1 || cin < 4 || cout < 4 || cin % 4 != 0 || cout % 4 != 0 || !x || !w_bf16 || !y) return HF_EINVAL;
    if (!bf_aligned16(x) || !bf_aligned16(w_bf16) || !bf_aligned16(y)) return HF_EINVAL;
    const int given = (gamma != nullptr) + (beta != nullptr) + (mean != nullptr) + (invstd != nullptr);
    if (given != 0 && given != 4) return HF_EINVAL;
    if (mode < 0 || mode > (kBfRelu | kBfElu) || (given == 0 && mode != 0)) return HF_EINVAL;
    hipStream_t st = as_stream(stream);
    // the column tile: 64 up to 64 outputs, 128 up to 128, 256 (eight waves) beyond
    if (cout <= 64) return launch_linear_bf16<2, 2>(rows, cin, cout, x, w_bf16, bias, gamma, beta, mean, invstd, mode, y, st);
    if (cout <= 128) return launch_linear_bf16<4, 2>(rows, cin, cout, x, w_bf16, bias, gamma, beta, mean, invstd, mode, y, st);
    return launch_linear_bf16<4, 4>(rows, cin, cout, x, w_bf16, bias, gamma, beta, mean, invstd, mode, y, st);
}
