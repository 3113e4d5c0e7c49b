// xconv.hip -- the two per-point products of PointCNN's X-Conv (hf/core/feature_extractors/pointcnn.py:16-151) for gfx950.
//
//   X-transform apply   F_X = X x F_*      pointcnn.py:133  tf.matmul(X, nn_fts_input): per representative point a (K,K)
//                                          matrix times the (K,C) block of lifted + gathered neighbour features
//   depthwise (1,K)     pointfly.py:437-457 depthwise_conv2d / the depthwise half of separable_conv2d with a (1,K) window
//                                          over a width-K input: out[c*M + m] = sum_w in[w][c] * W[w][c][m]
//
// In the reference both are library calls on tiny operands: a batched GEMM with 131 072 batches of 8x8 @ 8xC, and a
// depthwise convolution whose window covers its whole input.  The framework route costs a third of the PointCNN RPN
// step (batched-GEMM kernels at ~1.4 ms per layer, strided copies around every einsum).  Both are memory-bound by
// nature: every operand is read once and every result written once, the K*K (or K*M) coefficients of a point live in
// scalar registers / LDS.  fp32, multiply then add in index order (no FMA contraction), like the rest of the library.
//
// The two-kernel entries, the table gradient and every launcher live here.  The fused forward and F / Wd gradient kernels and the
// body of the X gradient are the templates of xconv_common.h: this file instantiates them with BN off, xconv_bn.hip with BN on.
#include "xconv_common.h"

namespace hf {

// out[r][i][ch] = sum_j X[r][i][j] * F[r][j][ch]   (TRANSPOSED: sum_j X[r][j][i] * F[r][j][ch], the dF of the backward)
// One wave per row at a time: the row's K*K coefficients are wave-uniform (scalar loads), lanes walk the channels.
template <int K, bool TRANSPOSED>
__global__ __launch_bounds__(kXcThreads) void xconv_apply_kernel(long long rows, int c, const float *__restrict__ x,
                                                                const float *__restrict__ f, float *__restrict__ out)
{
    const int lane = threadIdx.x & 63;
    const long long wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6)) +
                           static_cast<long long>(blockIdx.x) * (kXcThreads / 64);
    const long long nwaves = static_cast<long long>(gridDim.x) * (kXcThreads / 64);
    for (long long r = wave; r < rows; r += nwaves) {
        const float *xr = x + r * (K * K);
        float coef[K][K];
#pragma unroll
        for (int i = 0; i < K; ++i)
#pragma unroll
            for (int j = 0; j < K; ++j) coef[i][j] = TRANSPOSED ? xr[j * K + i] : xr[i * K + j];
        const float *fr = f + r * K * c;
        float *orow = out + r * K * c;
        for (int ch = lane; ch < c; ch += 64) {
            float v[K];
#pragma unroll
            for (int j = 0; j < K; ++j) v[j] = fr[static_cast<size_t>(j) * c + ch];
#pragma unroll
            for (int i = 0; i < K; ++i) {
                float acc = coef[i][0] * v[0];
#pragma unroll
                for (int j = 1; j < K; ++j) acc = acc + coef[i][j] * v[j];
                orow[static_cast<size_t>(i) * c + ch] = acc;
            }
        }
    }
}

// dX[r][i][j] = sum_ch dO[r][i][ch] * F[r][j][ch]: a wave per row; every lane accumulates the K*K products of its
// channels, the 64 partial matrices meet in LDS (stride K*K + 1: conflict-free both ways) and lane p sums entry p.
template <int K>
__global__ __launch_bounds__(kXcThreads) void xconv_dx_kernel(long long rows, int c, const float *__restrict__ grad_out,
                                                             const float *__restrict__ f, float *__restrict__ grad_x)
{
    extern __shared__ float lds[];
    constexpr int KK = K * K, STRIDE = KK + 1;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    float *mine = lds + static_cast<size_t>(w) * 64 * STRIDE;
    const long long wave = w + static_cast<long long>(blockIdx.x) * (kXcThreads / 64);
    const long long nwaves = static_cast<long long>(gridDim.x) * (kXcThreads / 64);
    for (long long r = wave; r < rows; r += nwaves) {
        const float *gr = grad_out + r * K * c;
        const float *fr = f + r * K * c;
        float acc[K][K];
#pragma unroll
        for (int i = 0; i < K; ++i)
#pragma unroll
            for (int j = 0; j < K; ++j) acc[i][j] = 0.f;
        for (int ch = lane; ch < c; ch += 64) {
            float g[K], v[K];
#pragma unroll
            for (int j = 0; j < K; ++j) { g[j] = gr[static_cast<size_t>(j) * c + ch]; v[j] = fr[static_cast<size_t>(j) * c + ch]; }
#pragma unroll
            for (int i = 0; i < K; ++i)
#pragma unroll
                for (int j = 0; j < K; ++j) acc[i][j] = acc[i][j] + g[i] * v[j];
        }
#pragma unroll
        for (int i = 0; i < K; ++i)
#pragma unroll
            for (int j = 0; j < K; ++j) mine[lane * STRIDE + i * K + j] = acc[i][j];
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        __builtin_amdgcn_wave_barrier();
        for (int p = lane; p < KK; p += 64) {
            float s = 0.f;
            for (int l = 0; l < 64; ++l) s = s + mine[l * STRIDE + p];
            grad_x[r * KK + p] = s;
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
}

// depthwise (1,K): y[r][ch*M + m] = sum_w x[r][w][ch] * W[w][ch][m]; one thread per (row, channel)
template <int K, int M>
__global__ __launch_bounds__(kXcThreads) void depthwise_fwd_kernel(long long rows, int c, const float *__restrict__ x,
                                                                  const float *__restrict__ wgt, float *__restrict__ y)
{
    const long long total = rows * c;
    for (long long g = static_cast<long long>(blockIdx.x) * kXcThreads + threadIdx.x; g < total;
         g += static_cast<long long>(gridDim.x) * kXcThreads) {
        const long long r = g / c;
        const int ch = static_cast<int>(g - r * c);
        float acc[M];
#pragma unroll
        for (int m = 0; m < M; ++m) acc[m] = 0.f;
#pragma unroll
        for (int w = 0; w < K; ++w) {
            const float xv = x[(r * K + w) * c + ch];
#pragma unroll
            for (int m = 0; m < M; ++m) acc[m] = acc[m] + xv * wgt[(static_cast<size_t>(w) * c + ch) * M + m];
        }
        store_m<M>(y, static_cast<size_t>(g) * M, acc);
    }
}

// dx[r][w][ch] = sum_m dy[r][ch*M + m] * W[w][ch][m]
template <int K, int M>
__global__ __launch_bounds__(kXcThreads) void depthwise_dx_kernel(long long rows, int c, const float *__restrict__ grad_y,
                                                                 const float *__restrict__ wgt, float *__restrict__ grad_x)
{
    const long long total = rows * c;
    for (long long g = static_cast<long long>(blockIdx.x) * kXcThreads + threadIdx.x; g < total;
         g += static_cast<long long>(gridDim.x) * kXcThreads) {
        const long long r = g / c;
        const int ch = static_cast<int>(g - r * c);
        float gy[M];
        load_m<M>(grad_y, static_cast<size_t>(g) * M, gy);
#pragma unroll
        for (int w = 0; w < K; ++w) {
            float acc = 0.f;
#pragma unroll
            for (int m = 0; m < M; ++m) acc = acc + gy[m] * wgt[(static_cast<size_t>(w) * c + ch) * M + m];
            grad_x[(r * K + w) * c + ch] = acc;
        }
    }
}

// Narrow layers (the X-transformation's own depthwise steps, pointcnn.py:107-131: c = K channels, depth multiplier K): with the
// grid a multiple of c threads, a thread keeps ONE channel for all its rows, and its K x M weights are loaded once into registers.
// The kernels above re-read them through the vector memory path for every row -- 64 loads per (row, channel) at K = M = 8: 85 us
// forward / 150 us input gradient for 131 072 rows x 8 channels (33 MB in, 33 MB out).  Same sums in the same order.
template <int K, int M, bool DX>
__global__ __launch_bounds__(kXcThreads) void depthwise_narrow_kernel(long long rows, int c, const float *__restrict__ in,
                                                                     const float *__restrict__ wgt, float *__restrict__ out)
{
    const long long tid = static_cast<long long>(blockIdx.x) * kXcThreads + threadIdx.x;
    const long long nthreads = static_cast<long long>(gridDim.x) * kXcThreads;   // a multiple of c (the launcher sees to it)
    const int ch = static_cast<int>(tid % c);
    float wr[K][M];
#pragma unroll
    for (int w = 0; w < K; ++w)
#pragma unroll
        for (int m = 0; m < M; ++m) wr[w][m] = wgt[(static_cast<size_t>(w) * c + ch) * M + m];
    for (long long r = tid / c; r < rows; r += nthreads / c) {
        if (!DX) {
            // y[r][ch*M + m] = sum_w x[r][w][ch] * W[w][ch][m]
            float acc[M];
#pragma unroll
            for (int m = 0; m < M; ++m) acc[m] = 0.f;
#pragma unroll
            for (int w = 0; w < K; ++w) {
                const float xv = in[(r * K + w) * c + ch];
#pragma unroll
                for (int m = 0; m < M; ++m) acc[m] = acc[m] + xv * wr[w][m];
            }
            store_m<M>(out, static_cast<size_t>(r * c + ch) * M, acc);
        } else {
            // dx[r][w][ch] = sum_m dy[r][ch*M + m] * W[w][ch][m]
            float gy[M];
            load_m<M>(in, static_cast<size_t>(r * c + ch) * M, gy);
#pragma unroll
            for (int w = 0; w < K; ++w) {
                float acc = 0.f;
#pragma unroll
                for (int m = 0; m < M; ++m) acc = acc + gy[m] * wr[w][m];
                out[(r * K + w) * c + ch] = acc;
            }
        }
    }
}

// grid for the narrow kernels: whole multiples of c threads, enough workgroups for the rows
static int narrow_grid(long long rows, int c)
{
    // kXcThreads * g must be a multiple of c: g a multiple of c / gcd(c, kXcThreads)
    int a = c, b = kXcThreads;
    while (b) { const int tmp = a % b; a = b; b = tmp; }
    const int unit = c / a;
    long long g = (rows * c + kXcThreads - 1) / kXcThreads;
    const long long cap = static_cast<long long>(kNumCU) * 8;
    if (g > cap) g = cap;
    g = (g + unit - 1) / unit * unit;
    return static_cast<int>(g);
}
constexpr int kNarrowMaxC = 64;

// dW[w][ch][m] = sum_r x[r][w][ch] * dy[r][ch*M + m]: thread (row chunk, channel) sums its rows in registers, then one
// atomic per coefficient and chunk (grad_w zero-filled by the entry point).  The order of the chunks is not fixed: the
// sum is reproducible to fp32 rounding, not bit for bit.
//
// `partial` != NULL (hf_depthwise_k_grad_ws): every chunk writes its K*c*M sums to partial[chunk][...] instead and a second
// kernel adds the chunks in a fixed order -- 512 chunks x 512 atomics on the same 16 cache lines were 50 us of a 60 us call
// for the X-transform's 8-channel layers, whatever the number of rows; deterministic as a bonus: the row slots of a block meet in
// a fixed order too (shuffles, or turns on the LDS slot), and tests/test_xconv_abi.py calls three times and compares the bits.
template <int K, int M>
__global__ __launch_bounds__(kXcThreads) void depthwise_dw_kernel(long long rows, int c, int rows_per_chunk,
                                                                 const float *__restrict__ x, const float *__restrict__ grad_y,
                                                                 float *__restrict__ grad_w, float *__restrict__ partial)
{
    // narrow layers (the X-transform has 8 channels): the threads a block has beyond the channels split the chunk's rows,
    // their partial sums meet in LDS, and the block issues ONE atomic per coefficient (8 x 8 x 8 coefficients hit by a
    // thousand blocks x 32 row slots each were 16 M atomics on 512 addresses: 7.6 ms)
    extern __shared__ float red[];   // [K * M][cw] when nrs > 1
    const int cw = c < kXcThreads ? c : kXcThreads, nrs = kXcThreads / cw;
    const int t = static_cast<int>(threadIdx.x);
    const int cl = t % cw, ch = blockIdx.x * cw + cl, rs = t / cw;
    const bool live = ch < c && rs < nrs;
    const long long r0 = static_cast<long long>(blockIdx.y) * rows_per_chunk + rs;
    const long long r1 = static_cast<long long>(blockIdx.y + 1) * rows_per_chunk < rows ? static_cast<long long>(blockIdx.y + 1) * rows_per_chunk : rows;
    float acc[K][M];
#pragma unroll
    for (int w = 0; w < K; ++w)
#pragma unroll
        for (int m = 0; m < M; ++m) acc[w][m] = 0.f;
    if (live) {
        for (long long r = r0; r < r1; r += nrs) {
            float gy[M];
            load_m<M>(grad_y, static_cast<size_t>(r * c + ch) * M, gy);
#pragma unroll
            for (int w = 0; w < K; ++w) {
                const float xv = x[(r * K + w) * c + ch];
#pragma unroll
                for (int m = 0; m < M; ++m) acc[w][m] = acc[w][m] + xv * gy[m];
            }
        }
    }
    float *mine = partial ? partial + static_cast<size_t>(blockIdx.y) * K * c * M : nullptr;
    if (nrs == 1) {
        if (live) {
#pragma unroll
            for (int w = 0; w < K; ++w)
#pragma unroll
                for (int m = 0; m < M; ++m) {
                    const size_t e = (static_cast<size_t>(w) * c + ch) * M + m;
                    if (mine) mine[e] = acc[w][m];
                    else atomicAdd(&grad_w[e], acc[w][m]);
                }
        }
        return;
    }
    // the row slots of a channel meet: inside a wave by xor-shuffles (power-of-two channel counts up to 32: the lanes of a
    // wave are 64 / cw row slots x cw channels), then one LDS slot per wave.  LDS atomics here -- 64 per thread, eight lanes of
    // a wave on every address -- were 13 us of serialised LDS work per block, the whole cost of the 8-channel layers.
    const bool shuffle = (cw & (cw - 1)) == 0 && cw <= 32;
    if (shuffle) {
        const int lane = t & 63, wave = t >> 6;
#pragma unroll
        for (int w = 0; w < K; ++w)
#pragma unroll
            for (int m = 0; m < M; ++m) {
                float v = live ? acc[w][m] : 0.f;
                for (int off = cw; off < 64; off <<= 1) v += __shfl_xor(v, off);
                if (lane < cw) red[(wave * K * M + w * M + m) * cw + lane] = v;
            }
        __syncthreads();
        for (int i = t; i < K * M * cw; i += kXcThreads) {
            float v = red[i];
#pragma unroll
            for (int wv = 1; wv < kXcThreads / 64; ++wv) v += red[wv * K * M * cw + i];
            const int wm = i / cw, c2 = blockIdx.x * cw + i % cw;
            if (c2 < c) {
                const size_t e = (static_cast<size_t>(wm / M) * c + c2) * M + wm % M;
                if (mine) mine[e] = v;
                else atomicAdd(&grad_w[e], v);
            }
        }
        return;
    }
    // other channel counts: the row slots take turns on the channel's LDS slot, slot 0 first (it holds every channel: cw = c here),
    // so the adds have a fixed order; LDS atomics did the same adds in whatever order the slots arrived
    for (int s = 0; s < nrs; ++s) {
        if (live && rs == s) {
#pragma unroll
            for (int w = 0; w < K; ++w)
#pragma unroll
                for (int m = 0; m < M; ++m) {
                    float *slot = &red[(w * M + m) * cw + cl];
                    *slot = s == 0 ? acc[w][m] : *slot + acc[w][m];
                }
        }
        __syncthreads();
    }
    for (int i = t; i < K * M * cw; i += kXcThreads) {
        const int wm = i / cw, c2 = blockIdx.x * cw + i % cw;
        if (c2 < c) {
            const size_t e = (static_cast<size_t>(wm / M) * c + c2) * M + wm % M;
            if (mine) mine[e] = red[i];
            else atomicAdd(&grad_w[e], red[i]);
        }
    }
}

// The fused X-transform apply + depthwise kernels (xconv_dw_fwd_kernel, xconv_dw_bwd_fw_kernel) are the templates of xconv_common.h,
// instantiated below with BN off at HF_XDW_DISPATCH, with and without GATHER.
// gradient w.r.t. X: dX[r][k][j] = sum_ch dF_X[r][k][ch] * F[r][j][ch] with dF_X rebuilt from grad_out and Wd on the fly;
// a wave per row.  The body is xc_bwd_x_body of xconv_common.h (shared with xconv_bn_bwd_x_kernel): Wd staged in LDS once per
// block, scalar row bases with 32-bit lane offsets, the next trip's loads in flight behind the current products, and the 64
// partial K x K matrices of the lanes summed by a halving exchange across the lanes (no LDS, 6 adds per entry).
// Dynamic LDS: xc_bwd_x_lds_bytes(c, 0, K * M).
template <int K, int M, bool GATHER>
__global__ __launch_bounds__(kXcThreads) void xconv_dw_bwd_x_kernel(long long rows, int c, int c0, const float *__restrict__ f,
                                                                   const float *__restrict__ fts, const int *__restrict__ idx, int n_src,
                                                                   int rows_per_cloud, const float *__restrict__ wd,
                                                                   const float *__restrict__ grad_out, float *__restrict__ grad_x)
{
    extern __shared__ float lds[];
    xc_bwd_x_body<K, M, GATHER, false>(rows, c, c0, f, nullptr, nullptr, nullptr, nullptr, fts, idx, n_src, rows_per_cloud, wd, grad_out,
                                       grad_x, lds);
}

// gradient w.r.t. the gathered feature table (GATHER mode): table row s collects, in ascending (row, slot) order (the CSR
// lists of hf_index_inverse, as hf_group_point_grad_gather sums them), the dF of every neighbour slot that read it,
//   dF[r][j][ch] = sum_k X[r][k][j] * (sum_m grad_out[r][ch*M+m] * Wd[k][ch][m]),
// rebuilt from grad_out on the fly with the multiply / add order of xconv_dw_bwd_fw_kernel: the (rows x K x c1) gradient
// of the gathered block is never written.  Every table row is written once (0 where nothing names it): no atomics, no zero fill.
// Layout (the arithmetic per element is that of the one-channel-per-lane form it replaces, so the bits are the same):
//   - a lane owns CPL consecutive channels of the table as channel pairs (4 channels for M = 1, else 2): a wave covers a
//     256-channel row with one 16-byte grad_out load per lane and list entry, and every product runs packed across a pair;
//   - a wave walks kFtsRows table rows at once and takes kFtsEntries list entries of each per trip: the entries (lane reads),
//     then the X columns and the grad_out rows of all kFtsRows * kFtsEntries slots are issued before the first sum.  Short
//     lists (2 at the encoder layers) no longer leave a wave with one load in flight;
//   - a trip's list entries are one load (a lane group per entry), and so are their X columns (X[r][k][j], k = 0..K-1, a lane
//     per coefficient), staged in the wave's LDS slots and read back as broadcasts (packed products take their scalar factor from a VGPR, see XcXRows);
//   - slots past a list's end load a clamped, valid entry and are skipped by a wave-uniform branch.
// `VEC`: c1 is a multiple of CPL and the tensors are 16-byte aligned: a lane's CPL * M floats of grad_out and its CPL results are
// whole 8- / 16-byte accesses, and a lane is live or dead as a whole.  Else single floats, each channel clamped and guarded.
// grad_out and grad_fts carry no __restrict__ on purpose: with it the compiler sinks the first entry's grad_out load past the
// LDS fence into that entry's branch, where it is issued last and waited for with every other load of the trip.
constexpr int kFtsRows = 2, kFtsEntries = 4;
typedef float f4 __attribute__((ext_vector_type(4)));

constexpr int xc_fts_pairs(int m) { return m == 1 ? 2 : 1; }   // channel pairs per lane

template <int K, int M, bool VEC>
__global__ __launch_bounds__(kXcThreads) void xconv_dw_bwd_fts_kernel(long long src_rows, int n_src, long long rows_per_cloud,
                                                                     int c, int c0, int rows_per_block,
                                                                     const float *__restrict__ x, const float *__restrict__ wd,
                                                                     const float *grad_out,
                                                                     const int *__restrict__ offsets, const int *__restrict__ entries,
                                                                     float *grad_fts)
{
    constexpr int NP = xc_fts_pairs(M), CPL = 2 * NP, T = kFtsRows, E = kFtsEntries, NF = CPL * M, CHUNK = NF % 4 == 0 ? 4 : 2;
    constexpr int KP = K <= 4 ? 4 : (K <= 8 ? 8 : 16), QPL = 64 / KP, NR = (T * E + QPL - 1) / QPL;   // X columns padded to KP floats
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6));
    const int lq = lane / KP, lk = lane % KP < K ? lane % KP : K - 1;
    const int c1 = c - c0, col0 = blockIdx.y * (64 * CPL), cf0 = col0 + lane * CPL;
    unsigned cc[CPL];   // the lane's channels in grad_out / wd, clamped to valid ones
    bool live[CPL];
#pragma unroll
    for (int i = 0; i < CPL; ++i) {
        live[i] = cf0 + i < c1;
        cc[i] = static_cast<unsigned>(c0 + (live[i] ? cf0 + i : (VEC ? col0 + i : c1 - 1)));
    }
    f2 w[K][NP][M];
#pragma unroll
    for (int k = 0; k < K; ++k)
#pragma unroll
        for (int p = 0; p < NP; ++p)
#pragma unroll
            for (int m = 0; m < M; ++m)
                w[k][p][m] = f2{wd[(static_cast<size_t>(k) * c + cc[2 * p]) * M + m], wd[(static_cast<size_t>(k) * c + cc[2 * p + 1]) * M + m]};
    __shared__ __attribute__((aligned(16))) float xs[kXcThreads / 64][T * E][KP];
    const long long s0 = static_cast<long long>(blockIdx.x) * rows_per_block;
    const long long s1 = s0 + rows_per_block < src_rows ? s0 + rows_per_block : src_rows;
    long long bb = s0 / n_src;
    for (long long sb = s0 + wave * T; sb < s1; sb += (kXcThreads / 64) * T) {
        int pos[T], hi[T];
        long long ebase[T];
        unsigned rbase[T];
        f2 acc[T][NP];
        bool more = false;
#pragma unroll
        for (int t = 0; t < T; ++t) {
            const long long s = sb + t < s1 ? sb + t : s1 - 1;
            while (s >= (bb + 1) * n_src) ++bb;
            const int pt = static_cast<int>(s - bb * n_src);
            const int *off = offsets + bb * (n_src + 1);
            ebase[t] = bb * rows_per_cloud * K;
            rbase[t] = static_cast<unsigned>(bb * rows_per_cloud);
            pos[t] = off[pt];
            hi[t] = sb + t < s1 ? off[pt + 1] : pos[t];   // a row past the block's end: an empty list, not stored
            more = more || pos[t] < hi[t];
#pragma unroll
            for (int p = 0; p < NP; ++p) acc[t][p] = f2{0.f, 0.f};
        }
        // lane l takes coefficient l % KP of entry l / KP: one load fetches 64 / KP list entries, a second one their X columns;
        // the entries reach the scalar side by lane reads.  The next trip's entries are loaded behind this trip's grad_out rows.
        auto load_slots = [&](int ahead, unsigned (&slot)[NR]) {
#pragma unroll
            for (int i = 0; i < NR; ++i) {
                const int q = i * QPL + lq < T * E ? i * QPL + lq : T * E - 1, u = q % E + ahead;
                int e = 0;
                long long eb = 0;
#pragma unroll
                for (int t = 0; t < T; ++t)
                    if (q / E == t) { e = pos[t] + u < hi[t] ? pos[t] + u : 0; eb = ebase[t]; }
                slot[i] = static_cast<unsigned>(entries[eb + e]);
            }
        };
        unsigned slot[NR], slot_next[NR];
        if (more) load_slots(0, slot);
        while (more) {
            unsigned rr[T * E];   // the entries' rows (fewer than 2^31, checked by the entry point)
            float xv[NR];
#pragma unroll
            for (int i = 0; i < NR; ++i) {
                const int q = i * QPL + lq < T * E ? i * QPL + lq : T * E - 1;
                unsigned rb = 0;
#pragma unroll
                for (int t = 0; t < T; ++t)
                    if (q / E == t) rb = rbase[t];
                xv[i] = x[static_cast<size_t>(rb + slot[i] / K) * (K * K) + lk * K + slot[i] % K];
#pragma unroll
                for (int j = 0; j < QPL; ++j) {
                    const int qj = i * QPL + j;
                    if (qj < T * E) rr[qj] = rbase[qj / E] + static_cast<unsigned>(__builtin_amdgcn_readlane(static_cast<int>(slot[i]), j * KP)) / K;
                }
            }
            f2 g[T * E][NP][M];
#pragma unroll
            for (int q = 0; q < T * E; ++q) {
                const float *gp = grad_out + static_cast<size_t>(rr[q]) * c * M;
                if constexpr (VEC) {
                    float flat[NF];
#pragma unroll
                    for (int i = 0; i < NF / CHUNK; ++i) {
                        if constexpr (CHUNK == 4) {
                            const f4 v = *reinterpret_cast<const f4 *>(gp + cc[0] * M + 4 * i);
                            flat[4 * i] = v.x; flat[4 * i + 1] = v.y; flat[4 * i + 2] = v.z; flat[4 * i + 3] = v.w;
                        } else {
                            const f2 v = *reinterpret_cast<const f2 *>(gp + cc[0] * M + 2 * i);
                            flat[2 * i] = v.x; flat[2 * i + 1] = v.y;
                        }
                    }
#pragma unroll
                    for (int p = 0; p < NP; ++p)
#pragma unroll
                        for (int m = 0; m < M; ++m) g[q][p][m] = f2{flat[2 * p * M + m], flat[(2 * p + 1) * M + m]};
                } else {
#pragma unroll
                    for (int p = 0; p < NP; ++p)
#pragma unroll
                        for (int m = 0; m < M; ++m) g[q][p][m] = f2{gp[cc[2 * p] * M + m], gp[cc[2 * p + 1] * M + m]};
                }
            }
            load_slots(E, slot_next);
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");   // the previous trip's reads are done
            __builtin_amdgcn_wave_barrier();
#pragma unroll
            for (int i = 0; i < NR; ++i) xs[wave][i * QPL + lq < T * E ? i * QPL + lq : T * E - 1][lane % KP] = xv[i];
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
            __builtin_amdgcn_wave_barrier();
            more = false;
#pragma unroll
            for (int t = 0; t < T; ++t) {
#pragma unroll
                for (int u = 0; u < E; ++u) {
                    const int q = t * E + u;
                    if (pos[t] + u >= hi[t]) continue;
                    const float *xr = xs[wave][q];
#pragma unroll
                    for (int p = 0; p < NP; ++p) {
                        f2 gfx[K];
#pragma unroll
                        for (int k = 0; k < K; ++k) {
                            f2 a = f2{0.f, 0.f};
#pragma unroll
                            for (int m = 0; m < M; ++m) a = a + g[q][p][m] * w[k][p][m];
                            gfx[k] = a;
                        }
                        f2 a = xr[0] * gfx[0];
#pragma unroll
                        for (int k = 1; k < K; ++k) a = a + xr[k] * gfx[k];
                        acc[t][p] = acc[t][p] + a;
                    }
                }
                pos[t] += E;
                more = more || pos[t] < hi[t];
            }
#pragma unroll
            for (int i = 0; i < NR; ++i) slot[i] = slot_next[i];
        }
#pragma unroll
        for (int t = 0; t < T; ++t) {
            if (sb + t >= s1) break;
            float *dst = grad_fts + static_cast<size_t>(sb + t) * c1 + cf0;
            if constexpr (VEC) {
                if (live[0]) {
                    if constexpr (NP == 2) *reinterpret_cast<f4 *>(dst) = f4{acc[t][0].x, acc[t][0].y, acc[t][1].x, acc[t][1].y};
                    else *reinterpret_cast<f2 *>(dst) = acc[t][0];
                }
            } else {
#pragma unroll
                for (int p = 0; p < NP; ++p) {
                    if (live[2 * p]) dst[2 * p] = acc[t][p].x;
                    if (live[2 * p + 1]) dst[2 * p + 1] = acc[t][p].y;
                }
            }
        }
    }
}

template <int K>
static int launch_apply(long long rows, int c, const float *x, const float *f, float *out, bool transposed, hipStream_t st)
{
    const int grid = grid_for(rows, kXcThreads / 64);
    if (transposed) hipLaunchKernelGGL((xconv_apply_kernel<K, true>), dim3(grid), dim3(kXcThreads), 0, st, rows, c, x, f, out);
    else hipLaunchKernelGGL((xconv_apply_kernel<K, false>), dim3(grid), dim3(kXcThreads), 0, st, rows, c, x, f, out);
    return launch_status();
}

template <int K>
static int launch_dx(long long rows, int c, const float *grad_out, const float *f, float *grad_x, hipStream_t st)
{
    const size_t lds = sizeof(float) * (kXcThreads / 64) * 64 * (K * K + 1);
    const int lrc = ensure_dynamic_lds(reinterpret_cast<const void *>(&xconv_dx_kernel<K>), lds);
    if (lrc != HF_OK) return lrc;
    hipLaunchKernelGGL((xconv_dx_kernel<K>), dim3(grid_for(rows, kXcThreads / 64)), dim3(kXcThreads), lds, st, rows, c, grad_out, f,
                       grad_x);
    return launch_status();
}

}  // namespace hf

using namespace hf;

HF_API int hf_xconv_apply(long long rows, int k, int c, const float *x, const float *f, float *out, hf_stream_t stream)
{
    if (rows < 0 || c <= 0 || !x || !f || !out) return HF_EINVAL;
    if (rows == 0) return HF_OK;
    switch (k) {
    case 4: return launch_apply<4>(rows, c, x, f, out, false, as_stream(stream));
    case 8: return launch_apply<8>(rows, c, x, f, out, false, as_stream(stream));
    default: return HF_EINVAL;   // K of the shipped configs is 8 (rpn_multiclass.config:67-112); other K: the caller's GEMM route
    }
}

HF_API int hf_xconv_apply_grad(long long rows, int k, int c, const float *x, const float *f, const float *grad_out,
                               float *grad_x, float *grad_f, hf_stream_t stream)
{
    if (rows < 0 || c <= 0 || !x || !f || !grad_out || (!grad_x && !grad_f)) return HF_EINVAL;
    if (rows == 0) return HF_OK;
    hipStream_t st = as_stream(stream);
    int rc = HF_OK;
#define HF_XC_CASE(KK)                                                                                                 \
    case KK:                                                                                                           \
        if (grad_f) rc = launch_apply<KK>(rows, c, x, grad_out, grad_f, true, st);                                     \
        if (rc == HF_OK && grad_x) rc = launch_dx<KK>(rows, c, grad_out, f, grad_x, st);                               \
        return rc;
    switch (k) {
        HF_XC_CASE(4)
        HF_XC_CASE(8)
    default: return HF_EINVAL;
    }
#undef HF_XC_CASE
}

// (k, m) pairs instantiated: the depthwise steps of the X-transform are (K, K) -> K*K with m = K; the separable
// convolutions use depth multipliers 1..4 (pointcnn.py:259-265)
#define HF_DW_DISPATCH(CALL)                                                                                           \
    if (k == 8 && m == 1) { CALL(8, 1) } else if (k == 8 && m == 2) { CALL(8, 2) } else if (k == 8 && m == 3) { CALL(8, 3) }      \
    else if (k == 8 && m == 4) { CALL(8, 4) } else if (k == 8 && m == 8) { CALL(8, 8) }                                 \
    else if (k == 4 && m == 1) { CALL(4, 1) } else if (k == 4 && m == 4) { CALL(4, 4) }                                 \
    else return HF_EINVAL;

HF_API int hf_depthwise_k(long long rows, int k, int c, int m, const float *x, const float *w, float *y, hf_stream_t stream)
{
    if (rows < 0 || c <= 0 || !x || !w || !y) return HF_EINVAL;
    if (rows == 0) return HF_OK;
    if (c <= kNarrowMaxC && k * m <= 64) {   // narrow layers: the thread's weights in registers
        const int ng = narrow_grid(rows, c);
#define HF_DW_NFWD(KK, MM) hipLaunchKernelGGL((depthwise_narrow_kernel<KK, MM, false>), dim3(ng), dim3(kXcThreads), 0, as_stream(stream), rows, c, x, w, y);
        HF_DW_DISPATCH(HF_DW_NFWD)
#undef HF_DW_NFWD
        return launch_status();
    }
    const int grid = grid_for(rows * c, kXcThreads);
#define HF_DW_FWD(KK, MM) hipLaunchKernelGGL((depthwise_fwd_kernel<KK, MM>), dim3(grid), dim3(kXcThreads), 0, as_stream(stream), rows, c, x, w, y);
    HF_DW_DISPATCH(HF_DW_FWD)
#undef HF_DW_FWD
    return launch_status();
}

static void dw_chunks(long long rows, int c, int &cblocks, int &rows_per_chunk, unsigned &nchunks)
{
    // enough chunks to fill the chip, few enough that the per-chunk tail stays a footnote; at least 64 rows per chunk
    cblocks = c < kXcThreads ? 1 : div_up(c, kXcThreads);
    long long chunks = (2 * kNumCU + cblocks - 1) / cblocks;
    if (chunks > (rows + 63) / 64) chunks = (rows + 63) / 64;
    if (chunks < 1) chunks = 1;
    if (chunks > rows) chunks = rows;
    if (chunks > 65535) chunks = 65535;
    rows_per_chunk = static_cast<int>((rows + chunks - 1) / chunks);
    nchunks = static_cast<unsigned>((rows + rows_per_chunk - 1) / rows_per_chunk);
}

HF_API size_t hf_depthwise_k_grad_workspace(long long rows, int k, int c, int m)
{
    if (rows <= 0 || k <= 0 || c <= 0 || m <= 0) return 0;
    int cblocks, rpc;
    unsigned nchunks;
    dw_chunks(rows, c, cblocks, rpc, nchunks);
    return sizeof(float) * static_cast<size_t>(nchunks) * k * c * m;
}

static int depthwise_k_grad_impl(long long rows, int k, int c, int m, const float *x, const float *w, const float *grad_y,
                                 float *grad_x, float *grad_w, float *partial, hipStream_t st)
{
    if (grad_w && (!partial || rows == 0)) {
        const int rc = hip_status(hipMemsetAsync(grad_w, 0, sizeof(float) * static_cast<size_t>(k) * c * m, st));
        if (rc != HF_OK) return rc;
    }
    if (rows == 0) return HF_OK;
    if (grad_x && c <= kNarrowMaxC && k * m <= 64) {
        const int ng = narrow_grid(rows, c);
#define HF_DW_NDX(KK, MM) hipLaunchKernelGGL((depthwise_narrow_kernel<KK, MM, true>), dim3(ng), dim3(kXcThreads), 0, st, rows, c, grad_y, w, grad_x);
        HF_DW_DISPATCH(HF_DW_NDX)
#undef HF_DW_NDX
        const int rc = launch_status();
        if (rc != HF_OK) return rc;
    } else if (grad_x) {
        const int grid = grid_for(rows * c, kXcThreads);
#define HF_DW_DX(KK, MM) hipLaunchKernelGGL((depthwise_dx_kernel<KK, MM>), dim3(grid), dim3(kXcThreads), 0, st, rows, c, grad_y, w, grad_x);
        HF_DW_DISPATCH(HF_DW_DX)
#undef HF_DW_DX
        const int rc = launch_status();
        if (rc != HF_OK) return rc;
    }
    if (grad_w) {
        int cblocks, rows_per_chunk;
        unsigned nchunks;
        dw_chunks(rows, c, cblocks, rows_per_chunk, nchunks);
        // block-level reduction when a block holds >= 2 row slots (one slot per wave on the shuffle path)
        const size_t lds = c <= kXcThreads / 2 ? sizeof(float) * static_cast<size_t>(k) * m * c * (((c & (c - 1)) == 0 && c <= 32) ? kXcThreads / 64 : 1) : 0;
        if (lds > 48 * 1024) return HF_EINVAL;
        const dim3 grid(cblocks, nchunks);
#define HF_DW_DW(KK, MM) hipLaunchKernelGGL((depthwise_dw_kernel<KK, MM>), grid, dim3(kXcThreads), lds, st, rows, c, rows_per_chunk, x, grad_y, grad_w, partial);
        HF_DW_DISPATCH(HF_DW_DW)
#undef HF_DW_DW
        if (partial) launch_partial_reduce(k * c * m, static_cast<int>(nchunks), partial, grad_w, st);
        return launch_status();
    }
    return HF_OK;
}

HF_API int hf_depthwise_k_grad(long long rows, int k, int c, int m, const float *x, const float *w, const float *grad_y,
                               float *grad_x, float *grad_w, hf_stream_t stream)
{
    if (rows < 0 || c <= 0 || !x || !w || !grad_y || (!grad_x && !grad_w)) return HF_EINVAL;
    return depthwise_k_grad_impl(rows, k, c, m, x, w, grad_y, grad_x, grad_w, nullptr, as_stream(stream));
}

HF_API int hf_depthwise_k_grad_ws(long long rows, int k, int c, int m, const float *x, const float *w, const float *grad_y,
                                  float *grad_x, float *grad_w, void *workspace, size_t workspace_bytes, hf_stream_t stream)
{
    if (rows < 0 || c <= 0 || !x || !w || !grad_y || (!grad_x && !grad_w)) return HF_EINVAL;
    if (grad_w && rows > 0 && (!workspace || workspace_bytes < hf_depthwise_k_grad_workspace(rows, k, c, m))) return HF_EWORKSPACE;
    return depthwise_k_grad_impl(rows, k, c, m, x, w, grad_y, grad_x, grad_w, grad_w ? static_cast<float *>(workspace) : nullptr,
                                 as_stream(stream));
}

// (k, m) supported by the fused X-apply + depthwise kernels: k = 8 with m = 1..4 (the separable convolutions of pointcnn.py:259-265
// under rpn_multiclass.config), and the RCNN's (4, 1), (4, 4), (12, 1), (12, 2)
#define HF_XDW_DISPATCH(CALL)                                                                                          \
    if (k == 8 && m == 1) { CALL(8, 1) } else if (k == 8 && m == 2) { CALL(8, 2) } else if (k == 8 && m == 3) { CALL(8, 3) }      \
    else if (k == 8 && m == 4) { CALL(8, 4) }                                                                          \
    else if (k == 4 && m == 1) { CALL(4, 1) } else if (k == 4 && m == 4) { CALL(4, 4) }   /* rcnn_multiclass.config:157-186: K = 4, 8, 12, 12 */ \
    else if (k == 12 && m == 1) { CALL(12, 1) } else if (k == 12 && m == 2) { CALL(12, 2) }                             \
    else return HF_EINVAL;

static void xdw_grid(long long rows, int c, dim3 &grid, int &rows_per_block, int blocks_per_cu = 8, int chunk = 64)
{
    const int cchunks = div_up(c, chunk);
    long long rchunks = (blocks_per_cu * kNumCU + cchunks - 1) / cchunks;   // ~8 blocks per CU in total (forward, dX)
    if (rchunks > (rows + 3) / 4) rchunks = (rows + 3) / 4;
    if (rchunks < 1) rchunks = 1;
    rows_per_block = static_cast<int>((rows + rchunks - 1) / rchunks);
    grid = dim3(static_cast<unsigned>((rows + rows_per_block - 1) / rows_per_block), cchunks);
}

// The forward kernel takes channel pairs: 128 channels per block column.  It indexes with 32-bit element offsets: the tensors
// it addresses by (row, neighbour) -- rows x k x c (F, or F_delta) and the feature table -- must hold fewer than 2^32 elements.  `V2`: pairs are read and written as 8-byte
// accesses, which needs c even (then every pair starts on an even element) and 8-byte aligned tensors.
bool hf::xdw_offsets_fit(long long rows, int k, int c, long long src_rows)
{
    return rows * k * static_cast<long long>(c) < (1ll << 32) && src_rows * static_cast<long long>(c) < (1ll << 32);
}

bool hf::xdw_v2(int c, std::initializer_list<const void *> ptrs)
{
    if (c & 1) return false;
    for (const void *p : ptrs)
        if (reinterpret_cast<uintptr_t>(p) & 7) return false;
    return true;
}

void hf::xdw_pair_grid(long long rows, int c, dim3 &grid, int &rpb, int blocks_per_cu) { xdw_grid(rows, c, grid, rpb, blocks_per_cu, 128); }

static int xdw_forward(long long rows, int k, int c, int c0, int m, const float *x, const float *f, const float *fts, const int *idx,
                       int n_src, int rows_per_cloud, const float *wd, float *out, hipStream_t st)
{
    if (!xdw_offsets_fit(rows, k, c, idx ? static_cast<long long>(rows / rows_per_cloud) * n_src : 0)) return HF_EINVAL;
    dim3 grid;
    int rpb;
    xdw_pair_grid(rows, c, grid, rpb, 8);
    const bool v2 = xdw_v2(c, {f, fts, out});
    const float *no_bn = nullptr;   // gamma, beta, mean, invstd of the BN = false instantiations
#define HF_XDW_FWD_V(KK, MM, V)                                                                                        \
    if (idx) hipLaunchKernelGGL((xconv_dw_fwd_kernel<KK, MM, true, V, false>), grid, dim3(kXcThreads), 0, st, rows, c, c0, rpb, x, f, no_bn, no_bn, no_bn, no_bn, fts, idx, n_src, rows_per_cloud, wd, out); \
    else hipLaunchKernelGGL((xconv_dw_fwd_kernel<KK, MM, false, V, false>), grid, dim3(kXcThreads), 0, st, rows, c, c0, rpb, x, f, no_bn, no_bn, no_bn, no_bn, fts, idx, n_src, rows_per_cloud, wd, out);
#define HF_XDW_FWD(KK, MM) if (v2) { HF_XDW_FWD_V(KK, MM, true) } else { HF_XDW_FWD_V(KK, MM, false) }
    HF_XDW_DISPATCH(HF_XDW_FWD)
#undef HF_XDW_FWD
#undef HF_XDW_FWD_V
    return launch_status();
}

// grid of xconv_dw_bwd_fw_kernel: every block ends in one sum per weight coefficient (an atomic on the same k*c*m addresses, or a
// row of the partial buffer): 4 blocks per CU, and at least 32 rows per block (one frame per GPU: the deep layers have a few
// hundred rows)
void hf::xdw_bwd_grid(long long rows, int c, dim3 &grid, int &rpb)
{
    xdw_grid(rows, c, grid, rpb, 4);
    if (rpb < 32 && rows > 32) { rpb = 32; grid.x = static_cast<unsigned>((rows + rpb - 1) / rpb); }
}

static int xdw_backward(long long rows, int k, int c, int c0, int m, const float *x, const float *f, const float *fts, const int *idx,
                        int n_src, int rows_per_cloud, const float *wd, const float *grad_out, float *grad_x, float *grad_f, float *grad_gathered,
                        float *grad_wd, hipStream_t st, float *wd_partial = nullptr)
{
    if (grad_wd && (!wd_partial || rows == 0)) {
        const int rc = hip_status(hipMemsetAsync(grad_wd, 0, sizeof(float) * static_cast<size_t>(k) * c * m, st));
        if (rc != HF_OK) return rc;
    }
    if (rows == 0) return HF_OK;
    if (!grad_wd) wd_partial = nullptr;
    if (grad_f || grad_wd || grad_gathered) {
        dim3 grid;
        int rpb;
        xdw_bwd_grid(rows, c, grid, rpb);
        const float *no_bn = nullptr;   // gamma, beta, mean, invstd of the BN = false instantiations
        float *no_sums = nullptr;       // their bn_partial
#define HF_XDW_BFW(KK, MM)                                                                                             \
        if (idx) hipLaunchKernelGGL((xconv_dw_bwd_fw_kernel<KK, MM, true, false>), grid, dim3(kXcThreads), 0, st, rows, c, c0, rpb, x, f, no_bn, no_bn, no_bn, no_bn, fts, idx, n_src, rows_per_cloud, wd, grad_out, grad_f, grad_gathered, grad_wd, wd_partial, no_sums); \
        else hipLaunchKernelGGL((xconv_dw_bwd_fw_kernel<KK, MM, false, false>), grid, dim3(kXcThreads), 0, st, rows, c, c0, rpb, x, f, no_bn, no_bn, no_bn, no_bn, fts, idx, n_src, rows_per_cloud, wd, grad_out, grad_f, grad_gathered, grad_wd, wd_partial, no_sums);
        HF_XDW_DISPATCH(HF_XDW_BFW)
#undef HF_XDW_BFW
        if (wd_partial) launch_partial_reduce(k * c * m, static_cast<int>(grid.x), wd_partial, grad_wd, st);
        const int rc = launch_status();
        if (rc != HF_OK) return rc;
    }
    if (grad_x) {
        const size_t lds = xc_bwd_x_lds_bytes(c, 0, k * m);   // the staged Wd: at most 16 KB
#define HF_XDW_BX(KK, MM)                                                                                              \
        if (idx) hipLaunchKernelGGL((xconv_dw_bwd_x_kernel<KK, MM, true>), dim3(grid_for(rows, kXcThreads / 64)), dim3(kXcThreads), lds, st, rows, c, c0, f, fts, idx, n_src, rows_per_cloud, wd, grad_out, grad_x); \
        else hipLaunchKernelGGL((xconv_dw_bwd_x_kernel<KK, MM, false>), dim3(grid_for(rows, kXcThreads / 64)), dim3(kXcThreads), lds, st, rows, c, c0, f, fts, idx, n_src, rows_per_cloud, wd, grad_out, grad_x);
        HF_XDW_DISPATCH(HF_XDW_BX)
#undef HF_XDW_BX
        return launch_status();
    }
    return HF_OK;
}

HF_API int hf_xconv_depthwise(long long rows, int k, int c, int m, const float *x, const float *f, const float *wd, float *out,
                              hf_stream_t stream)
{
    if (rows < 0 || c <= 0 || !x || !f || !wd || !out) return HF_EINVAL;
    if (rows == 0) return HF_OK;
    return xdw_forward(rows, k, c, c, m, x, f, nullptr, nullptr, 0, 1, wd, out, as_stream(stream));
}

HF_API int hf_xconv_depthwise_grad(long long rows, int k, int c, int m, const float *x, const float *f, const float *wd,
                                   const float *grad_out, float *grad_x, float *grad_f, float *grad_wd, hf_stream_t stream)
{
    if (rows < 0 || c <= 0 || !x || !f || !wd || !grad_out || (!grad_x && !grad_f && !grad_wd)) return HF_EINVAL;
    return xdw_backward(rows, k, c, c, m, x, f, nullptr, nullptr, 0, 1, wd, grad_out, grad_x, grad_f, nullptr, grad_wd, as_stream(stream));
}

// one row of k * c * m partial weight sums per row chunk of the F / Wd gradient kernel
HF_API size_t hf_xconv_depthwise_grad_workspace(long long rows, int k, int c, int m)
{
    if (rows <= 0 || k <= 0 || c <= 0 || m <= 0) return 0;
    dim3 grid;
    int rpb;
    xdw_bwd_grid(rows, c, grid, rpb);
    return sizeof(float) * static_cast<size_t>(grid.x) * k * c * m;
}

HF_API int hf_xconv_depthwise_grad_ws(long long rows, int k, int c, int m, const float *x, const float *f, const float *wd,
                                      const float *grad_out, float *grad_x, float *grad_f, float *grad_wd, void *workspace,
                                      size_t workspace_bytes, hf_stream_t stream)
{
    if (rows < 0 || c <= 0 || !x || !f || !wd || !grad_out || (!grad_x && !grad_f && !grad_wd)) return HF_EINVAL;
    if (grad_wd && rows > 0 && (!workspace || workspace_bytes < hf_xconv_depthwise_grad_workspace(rows, k, c, m))) return HF_EWORKSPACE;
    return xdw_backward(rows, k, c, c, m, x, f, nullptr, nullptr, 0, 1, wd, grad_out, grad_x, grad_f, nullptr, grad_wd, as_stream(stream),
                        grad_wd ? static_cast<float *>(workspace) : nullptr);
}

HF_API int hf_xconv_depthwise_gather(int b, int n_src, int rows_per_cloud, int k, int c0, int c1, int m, const float *x,
                                     const float *f_delta, const float *fts, const int *idx, const float *wd, float *out,
                                     hf_stream_t stream)
{
    if (b < 0 || n_src <= 0 || rows_per_cloud < 0 || c0 <= 0 || c0 % 64 != 0 || c1 <= 0) return HF_EINVAL;
    const long long rows = static_cast<long long>(b) * rows_per_cloud;
    if (rows == 0) return HF_OK;
    if (rows > 0x7fffffffll || !x || !f_delta || !fts || !idx || !wd || !out) return HF_EINVAL;
    return xdw_forward(rows, k, c0 + c1, c0, m, x, f_delta, fts, idx, n_src, rows_per_cloud, wd, out, as_stream(stream));
}

// Which route computes the feature table's gradient when a workspace is given: true = rebuilt per table row
// (xconv_dw_bwd_fts_kernel; the staging region of the workspace is never touched), false = staged in the workspace by
// xconv_dw_bwd_fw_kernel and summed by hf_group_point_grad_gather.  Direct reads k x (rows x c1 x m) floats of grad_out, mostly from
// the cache; staged writes and reads rows x k x c1.  Measured per shape as xconv_dw_bwd_fw_kernel + the table's kernel, direct
// against staged, us (scripts/probes/xconv_table_grad_timing.py, profiles/r06_xconv_table_grad_timing.txt):
//   lists of 8 and more: direct wins at every size -- 8 frames dec5 617 / 895, dec4 598 / 910, dec3 313 / 456, dec2 171 / 220,
//     dec1 66 / 72, dec0 33 / 38; one frame dec5 94 / 103 ... dec0 25 / 29
//   short lists (2 .. 4), where a wave has little in flight per table row:
//     staged block of 8 MiB and less (one frame's encoder, all latency): direct, one launch fewer -- 31 / 33, 27 / 30, 22 / 26
//     m <= 2 and a block well past the caches: direct -- m = 1: enc1 at 8 frames (268 MB) 183 / 253, the RCNN's second layer at
//       128 / 512 RoIs (268 MB / 1.07 GB) 190 / 244, 710 / 943, its fourth at 512 RoIs (201 MB) 254 / 310; m = 2: its third
//       (101 / 403 MB) 157 / 193, 502 / 746
//     otherwise staged -- m = 1 at 17 .. 50 MB 36 / 33, 48 / 40, 87 / 74; m = 2 at 34 and 67 MB (enc3, enc2) 53 / 46, 82 / 72;
//       m = 4, where grad_out is four times the block (the RCNN's first layer, k 4, 570 MB / 2.3 GB) 672 / 592, 3010 / 2345
//   the 80 MiB lies between the largest block where staging won (64 MiB) and the smallest where it lost (96 MiB)
bool hf::xdw_fts_direct(long long rows, int n_src, int rows_per_cloud, int k, int c1, int m)
{
    if (static_cast<long long>(rows_per_cloud) * k >= 8ll * n_src) return true;
    const long long staged = rows * k * c1 * static_cast<long long>(sizeof(float));
    return staged <= (8ll << 20) || (m <= 2 && staged >= (80ll << 20));
}

// rows = b * rows_per_cloud stays below 2^31 (checked by the entry point): the kernel keeps a list entry's row in 32 bits
int hf::xdw_table_grad(long long src_rows, int n_src, int rows_per_cloud, int k, int c, int c0, int m, const float *x, const float *wd,
                          const float *grad_out, const int *offsets, const int *entries, float *grad_fts, hipStream_t st)
{
    const int c1 = c - c0, cpl = 2 * xc_fts_pairs(m);
    dim3 grid;
    int rpb;
    xdw_grid(src_rows, c1, grid, rpb, 8, 64 * cpl);
    const bool vec = c1 % cpl == 0 && ((reinterpret_cast<uintptr_t>(grad_out) | reinterpret_cast<uintptr_t>(grad_fts)) & 15) == 0;
#define HF_XDW_FTS_V(KK, MM, V) hipLaunchKernelGGL((xconv_dw_bwd_fts_kernel<KK, MM, V>), grid, dim3(kXcThreads), 0, st, src_rows, n_src, static_cast<long long>(rows_per_cloud), c, c0, rpb, x, wd, grad_out, offsets, entries, grad_fts);
#define HF_XDW_FTS(KK, MM) if (vec) { HF_XDW_FTS_V(KK, MM, true) } else { HF_XDW_FTS_V(KK, MM, false) }
    HF_XDW_DISPATCH(HF_XDW_FTS)
#undef HF_XDW_FTS
#undef HF_XDW_FTS_V
    return launch_status();
}

// [gradient of the gathered block: rows x k x c1][partial depthwise-weight gradients: row chunks x k x (c0+c1) x m]
size_t hf::xdw_gathered_bytes(int b, int rows_per_cloud, int k, int c1)
{
    return (sizeof(float) * static_cast<size_t>(b) * rows_per_cloud * k * c1 + 255) & ~static_cast<size_t>(255);
}

// the plan, the tail and the empty batch of the two gather-mode gradient entries (this file's and xconv_bn.hip's; xconv_common.h)
XdwGradPlan hf::xdw_grad_plan(int b, int n_src, int rows_per_cloud, int k, int c1, int m, const float *grad_fts, void *workspace)
{
    XdwGradPlan plan;
    plan.direct = grad_fts && (!workspace || xdw_fts_direct(static_cast<long long>(b) * rows_per_cloud, n_src, rows_per_cloud, k, c1, m));
    if (grad_fts && workspace && HF_DIAG_INT("HF_XDW_FTS_ROUTE", 0) != 0) plan.direct = HF_DIAG_INT("HF_XDW_FTS_ROUTE", 0) == 2;   // 1: staged, 2: direct
    plan.gathered = (grad_fts && !plan.direct) ? static_cast<float *>(workspace) : nullptr;
    plan.wd_partial = workspace ? reinterpret_cast<float *>(static_cast<unsigned char *>(workspace) + xdw_gathered_bytes(b, rows_per_cloud, k, c1)) : nullptr;
    return plan;
}

int hf::xdw_grad_table(const XdwGradPlan &plan, int b, int n_src, int rows_per_cloud, int k, int c0, int c1, int m, const float *x,
                       const float *wd, const float *grad_out, const int *offsets, const int *entries, float *grad_fts, hf_stream_t stream)
{
    if (plan.gathered) return hf_group_point_grad_gather(b, n_src, c1, rows_per_cloud, k, c1, 0, plan.gathered, offsets, entries, grad_fts, stream);
    if (plan.direct)
        return xdw_table_grad(static_cast<long long>(b) * n_src, n_src, rows_per_cloud, k, c0 + c1, c0, m, x, wd, grad_out, offsets, entries, grad_fts,
                              as_stream(stream));
    return HF_OK;
}

int hf::xdw_grad_empty(int b, int n_src, int k, int c0, int c1, int m, float *grad_fts, float *grad_wd, hipStream_t st)
{
    int rc = HF_OK;
    if (grad_wd) rc = hip_status(hipMemsetAsync(grad_wd, 0, sizeof(float) * static_cast<size_t>(k) * (c0 + c1) * m, st));
    if (rc == HF_OK && grad_fts && b > 0) rc = hip_status(hipMemsetAsync(grad_fts, 0, sizeof(float) * static_cast<size_t>(b) * n_src * c1, st));
    return rc;
}

HF_API size_t hf_xconv_depthwise_gather_grad_workspace(int b, int rows_per_cloud, int k, int c0, int c1, int m)
{
    if (b <= 0 || rows_per_cloud <= 0 || k <= 0 || c0 <= 0 || c1 <= 0 || m <= 0) return 0;
    dim3 grid;
    int rpb;
    xdw_bwd_grid(static_cast<long long>(b) * rows_per_cloud, c0 + c1, grid, rpb);
    return xdw_gathered_bytes(b, rows_per_cloud, k, c1) + sizeof(float) * static_cast<size_t>(grid.x) * k * (c0 + c1) * m;
}

HF_API int hf_xconv_depthwise_gather_grad(int b, int n_src, int rows_per_cloud, int k, int c0, int c1, int m, const float *x,
                                          const float *f_delta, const float *fts, const int *idx, const float *wd,
                                          const float *grad_out, const int *offsets, const int *entries, float *grad_x,
                                          float *grad_f_delta, float *grad_fts, float *grad_wd, void *workspace,
                                          size_t workspace_bytes, hf_stream_t stream)
{
    if (b < 0 || n_src <= 0 || rows_per_cloud < 0 || c0 <= 0 || c0 % 64 != 0 || c1 <= 0 || !x || !f_delta || !fts || !idx || !wd ||
        !grad_out || static_cast<long long>(b) * rows_per_cloud > 0x7fffffffll ||
        (!grad_x && !grad_f_delta && !grad_fts && !grad_wd))
        return HF_EINVAL;
    if (grad_fts && (!offsets || !entries)) return HF_EINVAL;
    if (workspace && workspace_bytes < hf_xconv_depthwise_gather_grad_workspace(b, rows_per_cloud, k, c0, c1, m)) return HF_EWORKSPACE;
    hipStream_t st = as_stream(stream);
    if (b == 0 || rows_per_cloud == 0) return xdw_grad_empty(b, n_src, k, c0, c1, m, grad_fts, grad_wd, st);
    const XdwGradPlan plan = xdw_grad_plan(b, n_src, rows_per_cloud, k, c1, m, grad_fts, workspace);
    if (grad_x || grad_f_delta || grad_wd || plan.gathered) {
        const int rc = xdw_backward(static_cast<long long>(b) * rows_per_cloud, k, c0 + c1, c0, m, x, f_delta, fts, idx, n_src, rows_per_cloud, wd, grad_out,
                                    grad_x, grad_f_delta, plan.gathered, grad_wd, st, plan.wd_partial);
        if (rc != HF_OK) return rc;
    }
    return xdw_grad_table(plan, b, n_src, rows_per_cloud, k, c0, c1, m, x, wd, grad_out, offsets, entries, grad_fts, stream);
}
