// linear_bf16_train.hip -- what training the wide dense layers on the bf16 matrix cores adds to linear_bf16.hip: the weight gradient
// (hf_linear_bf16_wgrad) and the transposing weight conversion (hf_f32_to_bf16_transpose) that lets the input gradient
// dx = bf16(g) . (W^T)^T run as hf_linear_bf16_fwd_eval.
//
// Weight gradient.  dW (cout, cin) = bf16(g)^T (cout, rows) . bf16(x) (rows, cin), fp32 accumulation.  g and x stay fp32 in memory and
// are rounded (nearest even, pack_bf16x2) between the global load and the LDS store.  The reduction runs over rows, which is the slow
// axis of both operands in memory, while a lane of v_mfma_f32_16x16x32_bf16 wants 8 consecutive k of one channel.
// A workgroup of 2 x WN waves owns 128 outputs x 64 WN inputs of dW for one chunk of rows; a wave owns 64 x 64 as 4 x 4 accumulator
// tiles.  The MFMA's A operand is the x tile and its B operand the g tile, so that D holds, per lane, one output channel and four
// CONSECUTIVE input channels (D row = 4 (lane >> 4) + reg -> cin, D column = lane & 15 -> cout): the partial tile is stored sixteen
// bytes at a time.  A stage is 64 rows (two k-steps); the next stage's loads are in flight during the MFMAs.  The chunk partials go
// to the workspace as [chunk][cout][cin] and are summed in a fixed order by the reduction kernel of hf_linear_wgrad (gemm.hip); one
// chunk writes dW directly.  No atomics: two calls give the same bits.
//
// Staging: the tile is stored as it arrives, [row][channel] as bf16 (one 8-byte LDS store per 16-byte load), and the operands are read
// with the gfx950 transposed LDS read ds_read_b64_tr_b16: lane 4q + p of a 16-lane group supplies the address of row q, channels
// 4p .. 4p + 3 of a 4-row x 16-channel block and receives the 4 rows of channel (lane & 15).  Group g takes rows 4g .. 4g + 3 for the
// low and rows 16 + 4g .. for the high half of its 8-element fragment; both operands use this row -> k map, so the order of k inside
// a k-step is immaterial to the product.  Every address is 8-byte aligned and inside the staged tile, and no lane is masked (EXEC is
// all ones in the loop: rows past the chunk and channels past cout / cin are staged as zeros by load4_guarded instead).
// Bank rule: a 32-lane half reads 8 consecutive rows x 32 bytes; the row stride is 32 bytes more than a multiple of 256 bytes
// (288 bytes for 128 channels, 544 for 256), so the 8 rows fall on 8 different 8-bank groups: conflict-free.
// Chosen by measurement against the other staging, transposing while storing (8 rows x 4 channels per thread packed into four
// ds_write_b128 of a [channel][row] image, one ds_read_b128 per fragment), built once from the same kernel and giving the same bits:
// partial kernels alone, median of 5 rounds on one MI355X, transposed read / transposing store: 131072 x 256 x 256 82 / 90 us,
// 131072 x 256 x 320 103 / 125, 131072 x 256 x 512 110 / 133, 16384 x 256 x 512 17.6 / 21.2, 4096 x 256 x 320 12.4 / 16.3,
// 65536 x 512 x 2688 485 / 597.  The transposing store took 9 to 38 % longer on every shape.  The figures are kept in
// profiles/bf16_training_timing.json ("wgrad_staging"); the other variant is not in the tree, so they cannot be regenerated from it.
#include "bf16_common.h"
#include "gemm_common.h"
#include "hf_common.h"

namespace hf {

constexpr int kBwOut = 128;             // output channels (rows of dW) per workgroup tile
constexpr int kBwKC = 64;               // rows of g / x per LDS stage: two MFMA k-steps
constexpr int kBwPad = 16;              // bf16 elements (32 bytes) added to an LDS row: see the bank rule above
constexpr int kBwMinChunk = 256;        // rows per chunk at least
constexpr int kBwMaxChannels = 32768;   // cout, cin: cout * cin fits the reduction's int

template <int WN>
struct alignas(16) BwLds {
    uint16_t Gs[kBwKC * (kBwOut + kBwPad)];
    uint16_t Xs[kBwKC * (64 * WN + kBwPad)];
};

typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));

// the 8-element fragment of a lane for the 32-row k-step that starts at `base` (the lane's own row and channel offset applied)
__device__ __forceinline__ bf16x8 tr_fragment(const uint16_t *base, int stride)
{
    typedef s16x4 __attribute__((address_space(3))) *lds_ptr;
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_ptr)(base));
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_ptr)(base + 16 * stride));
    const s16x8 v = { lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3] };
    return __builtin_bit_cast(bf16x8, v);
}

template <int WN>
__global__ __launch_bounds__(128 * WN) __attribute__((amdgpu_waves_per_eu(2))) void wgrad_bf16_kernel(long long rows, int cout, int cin, int ntiles, int tiles,
                                                                                                 long long rows_per_chunk,
                                                                                                 const float *__restrict__ G,
                                                                                                 const float *__restrict__ X,
                                                                                                 float *__restrict__ partial)
{
    constexpr int THREADS = 128 * WN, BN = 64 * WN;
    constexpr int XQ = BN / 4;                    // channel quads of an x row; the g tile has 32
    constexpr int SG = kBwOut + kBwPad, SX = BN + kBwPad;   // LDS row strides in elements
    __shared__ BwLds<WN> lds;

    // consecutive workgroups of one chunk (they re-read its rows) on one XCD, as linear_bf16_kernel numbers its tiles
    const unsigned per_xcd = gridDim.x / kNumXCD;
    const unsigned id = blockIdx.x < per_xcd * kNumXCD ? (blockIdx.x % kNumXCD) * per_xcd + blockIdx.x / kNumXCD : blockIdx.x;
    const long long chunk = id / tiles;
    const int tile = static_cast<int>(id % tiles);
    const int o0 = (tile / ntiles) * kBwOut, i0 = (tile % ntiles) * BN;
    const long long r0 = chunk * rows_per_chunk;
    const long long r1 = r0 + rows_per_chunk < rows ? r0 + rows_per_chunk : rows;

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int wm = wave & 1, wn = wave >> 1;
    const bool stages_g = THREADS == 256 || t < 256;       // whole waves: the g tile has 8 x 32 units of 8 rows x 4 channels
    const int gq = (t & 31) * 4, grg = ((t >> 5) & 7) * 8;
    const int xq = (t % XQ) * 4, xrg = (t / XQ) * 8;

    float4 gr[8], xr[8];
    auto fetch = [&](long long rt) {
        if (stages_g) {
#pragma unroll
            for (int i = 0; i < 8; ++i) gr[i] = load4_guarded<true>(G, rt + grg + i, r1, o0 + gq, cout);
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) xr[i] = load4_guarded<true>(X, rt + xrg + i, r1, i0 + xq, cin);
    };

    f32x4 acc[4][4];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) acc[mt][nt] = f32x4{ 0.f, 0.f, 0.f, 0.f };

    // transposed read: row 4 (lane >> 4) + ((lane >> 2) & 3), channels 4 (lane & 3) .. + 3 of the wave's 64-channel slice
    const int frow = 4 * (lane >> 4) + ((lane >> 2) & 3), fcol = 4 * (lane & 3);
    const uint16_t *gf = lds.Gs + frow * SG + wm * 64 + fcol;
    const uint16_t *xf = lds.Xs + frow * SX + wn * 64 + fcol;

    fetch(r0);
    for (long long rt = r0; rt < r1; rt += kBwKC) {
        if (stages_g) {
#pragma unroll
            for (int i = 0; i < 8; ++i)
                *reinterpret_cast<uint2 *>(&lds.Gs[(grg + i) * SG + gq]) = make_uint2(pack_bf16x2(gr[i].x, gr[i].y), pack_bf16x2(gr[i].z, gr[i].w));
        }
#pragma unroll
        for (int i = 0; i < 8; ++i)
            *reinterpret_cast<uint2 *>(&lds.Xs[(xrg + i) * SX + xq]) = make_uint2(pack_bf16x2(xr[i].x, xr[i].y), pack_bf16x2(xr[i].z, xr[i].w));
        __syncthreads();
        if (rt + kBwKC < r1) fetch(rt + kBwKC);  // in flight during the MFMAs below
#pragma unroll
        for (int ks = 0; ks < kBwKC / 32; ++ks) {
            bf16x8 a[4], b[4];
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) a[nt] = tr_fragment(xf + ks * 32 * SX + nt * 16, SX);
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) b[mt] = tr_fragment(gf + ks * 32 * SG + mt * 16, SG);
#pragma unroll
            for (int mt = 0; mt < 4; ++mt)
#pragma unroll
                for (int nt = 0; nt < 4; ++nt)
                    acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[nt], b[mt], acc[mt][nt], 0, 0, 0);
        }
        __syncthreads();
    }

    // this lane holds dW[o][i .. i + 3] of the chunk in acc[mt][nt]; cin % 4 == 0: the four are inside or outside together
    float *out = partial + static_cast<size_t>(chunk) * cout * cin;
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
        const int o = o0 + wm * 64 + mt * 16 + (lane & 15);
        if (o >= cout) continue;
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
            const int i = i0 + wn * 64 + nt * 16 + (lane >> 4) * 4;
            if (i >= cin) continue;
            *reinterpret_cast<float4 *>(out + static_cast<size_t>(o) * cin + i) =
                make_float4(acc[mt][nt][0], acc[mt][nt][1], acc[mt][nt][2], acc[mt][nt][3]);
        }
    }
}

// The launch plan, which the workspace query and the launcher must agree on: 128-input tiles up to 128 inputs and 256-input tiles
// (eight waves) beyond; about three workgroups per CU in all, a chunk being at least 256 rows and a multiple of the 64-row stage.
struct BwPlan {
    int wn, mtiles, ntiles, chunks;
    long long rows_per_chunk;
};

static BwPlan bw_plan(long long rows, int cout, int cin)
{
    BwPlan p;
    p.wn = cin > 128 ? 4 : 2;
    p.mtiles = div_up(cout, kBwOut);
    p.ntiles = div_up(cin, 64 * p.wn);
    long long want = static_cast<long long>(kNumCU) * 3 / (p.mtiles * p.ntiles);
    if (want < 1) want = 1;
    long long rpc = (rows + want - 1) / want;
    rpc = (rpc + kBwKC - 1) / kBwKC * kBwKC;
    if (rpc < kBwMinChunk) rpc = kBwMinChunk;
    p.rows_per_chunk = rpc;
    p.chunks = static_cast<int>((rows + rpc - 1) / rpc);
    return p;
}

// dst (cols, rows) = bf16(src (rows, cols))^T through a 32 x 32 LDS tile: a 32-lane row of the workgroup reads 128 consecutive bytes
// of a src row and writes 64 consecutive bytes of a dst row.  The stride of 33 floats keeps the column reads off one bank.
constexpr int kTrTile = 32;
__global__ __launch_bounds__(256) void f32_to_bf16_transpose_kernel(int rows, int cols, int col_tiles, const float *__restrict__ src,
                                                                    uint16_t *__restrict__ dst)
{
    __shared__ float tile[kTrTile][kTrTile + 1];
    const int r0 = static_cast<int>(blockIdx.x / col_tiles) * kTrTile, c0 = static_cast<int>(blockIdx.x % col_tiles) * kTrTile;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
#pragma unroll
    for (int p = 0; p < kTrTile; p += 8) {
        const int r = r0 + ty + p, c = c0 + tx;
        tile[ty + p][tx] = r < rows && c < cols ? src[static_cast<size_t>(r) * cols + c] : 0.0f;
    }
    __syncthreads();
#pragma unroll
    for (int p = 0; p < kTrTile; p += 8) {
        const int c = c0 + ty + p, r = r0 + tx;
        if (c < cols && r < rows) dst[static_cast<size_t>(c) * rows + r] = static_cast<uint16_t>(pack_bf16x2(tile[tx][ty + p], 0.0f) & 0xffffu);
    }
}

}  // namespace hf

using namespace hf;

HF_API int hf_f32_to_bf16_transpose(int rows, int cols, const float *src, uint16_t *dst, hf_stream_t stream)
{
    if (rows < 1 || cols < 1 || !src || !dst) return HF_EINVAL;
    if (reinterpret_cast<uintptr_t>(src) % 4 != 0 || reinterpret_cast<uintptr_t>(dst) % 2 != 0) return HF_EINVAL;
    const int col_tiles = div_up(cols, kTrTile);
    const long long blocks = static_cast<long long>(div_up(rows, kTrTile)) * col_tiles;
    if (blocks > 0x7fffffffLL) return HF_EINVAL;
    hipLaunchKernelGGL(f32_to_bf16_transpose_kernel, dim3(static_cast<unsigned>(blocks)), dim3(256), 0, as_stream(stream), rows, cols, col_tiles,
                       src, dst);
    return launch_status();
}

static bool bw_shape_ok(long long rows, int cout, int cin)
{
    return rows >= 1 && cout >= 4 && cin >= 4 && cout % 4 == 0 && cin % 4 == 0 && cout <= kBwMaxChannels && cin <= kBwMaxChannels;
}

HF_API size_t hf_linear_bf16_wgrad_workspace(long long rows, int cout, int cin)
{
    if (!bw_shape_ok(rows, cout, cin)) return 0;
    return sizeof(float) * static_cast<size_t>(bw_plan(rows, cout, cin).chunks) * cout * cin;
}

HF_API int hf_linear_bf16_wgrad(long long rows, int cout, int cin, const float *grad_z, const float *x, float *grad_weight, void *workspace,
                                size_t workspace_bytes, hf_stream_t stream)
{
    if (!bw_shape_ok(rows, cout, cin) || !grad_z || !x || !grad_weight || !workspace) return HF_EINVAL;
    if (!bf_aligned16(grad_z) || !bf_aligned16(x) || !bf_aligned16(grad_weight) || !bf_aligned16(workspace)) return HF_EINVAL;
    if (workspace_bytes < hf_linear_bf16_wgrad_workspace(rows, cout, cin)) return HF_EINVAL;
    const BwPlan p = bw_plan(rows, cout, cin);
    const int tiles = p.mtiles * p.ntiles;
    hipStream_t st = as_stream(stream);
    float *partial = p.chunks == 1 ? grad_weight : static_cast<float *>(workspace);
    const dim3 grid(static_cast<unsigned>(tiles) * p.chunks);
    if (p.wn == 2)
        hipLaunchKernelGGL((wgrad_bf16_kernel<2>), grid, dim3(256), 0, st, rows, cout, cin, p.ntiles, tiles, p.rows_per_chunk, grad_z, x, partial);
    else
        hipLaunchKernelGGL((wgrad_bf16_kernel<4>), grid, dim3(512), 0, st, rows, cout, cin, p.ntiles, tiles, p.rows_per_chunk, grad_z, x, partial);
    if (p.chunks > 1) launch_partial_reduce(cout * cin, p.chunks, partial, grad_weight, st);
    return launch_status();
}
