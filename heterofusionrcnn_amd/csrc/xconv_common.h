// xconv_common.h -- the fused X-Conv kernels that xconv.hip instantiates as they are and xconv_bn.hip with the lifting branch's last
// BatchNorm folded in (`BN`): the device helpers of the channel-pair / lane-per-channel mappings, the kernel templates of the three
// passes, and the launch geometry, gradient plan and table-gradient launcher that xconv.hip defines.
#pragma once
#include "hf_common.h"

#include <initializer_list>
#include <type_traits>

namespace hf {

// The M consecutive floats a (row, channel) pair owns in a (rows, C*M) tensor.  As M scalar accesses a wave's instruction touches
// 64 x 4 bytes at a stride of 4 M bytes -- every cache line of the row is visited M times (the K = 4, M = 4 layer of the RCNN wrote
// its 2.4 GB at 1.2 TB/s that way); as ONE 8- / 16-byte access per lane the instruction covers a contiguous range.  `base` is
// the tensor's first element (a kernel argument: the alignment test is wave-uniform).
template <int M>
__device__ __forceinline__ void store_m(float *base, size_t elem, const float (&v)[M])
{
    float *p = base + elem;
    if constexpr (M == 4 || M == 8) {
        if ((reinterpret_cast<uintptr_t>(base) & 15) == 0) {
#pragma unroll
            for (int q = 0; q < M / 4; ++q) reinterpret_cast<float4 *>(p)[q] = make_float4(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]);
            return;
        }
    } else if constexpr (M == 2) {
        if ((reinterpret_cast<uintptr_t>(base) & 7) == 0) { *reinterpret_cast<float2 *>(p) = make_float2(v[0], v[1]); return; }
    }
#pragma unroll
    for (int m = 0; m < M; ++m) p[m] = v[m];
}
template <int M>
__device__ __forceinline__ void load_m(const float *base, size_t elem, float (&v)[M])
{
    const float *p = base + elem;
    if constexpr (M == 4 || M == 8) {
        if ((reinterpret_cast<uintptr_t>(base) & 15) == 0) {
#pragma unroll
            for (int q = 0; q < M / 4; ++q) {
                const float4 t = reinterpret_cast<const float4 *>(p)[q];
                v[4 * q] = t.x; v[4 * q + 1] = t.y; v[4 * q + 2] = t.z; v[4 * q + 3] = t.w;
            }
            return;
        }
    } else if constexpr (M == 2) {
        if ((reinterpret_cast<uintptr_t>(base) & 7) == 0) { const float2 t = *reinterpret_cast<const float2 *>(p); v[0] = t.x; v[1] = t.y; return; }
    }
#pragma unroll
    for (int m = 0; m < M; ++m) v[m] = p[m];
}


constexpr int kXcThreads = 256;

// Channel pairs: a lane owns channels (ch, ch + 1), ch even, so a wave covers 128 channels and every product runs as ONE packed
// f32 op on the pair (v_pk_mul_f32 / v_pk_add_f32 round each half like the scalar op; -ffp-contract=off keeps them unfused).
// Packing runs across channels only: every output element keeps its own multiply-then-add sequence in index order.
typedef float f2 __attribute__((ext_vector_type(2)));

// Where a lane's channel pair comes from.  c0 is a multiple of 64, so a 128-channel wave may straddle the lifted / gathered
// split at lane 32: the source is picked per lane by select (base pointer and row offset), with no branch around the loads.
// Element offsets are 32-bit (the launcher checks the tensor sizes).  A lane past the last channel reads a clamped, valid
// pair and stores nothing; with c odd (`V2` false) the pair is read as two floats, the second one only while ch + 1 < c.
struct XcPair {
    const float *base;   // f + ch (lifted) or fts + ch - c0 (gathered)
    unsigned hi;         // offset of the second channel: 1, or 0 where ch + 1 is past the end
    bool gathered, live, hi_live;
};

__device__ __forceinline__ XcPair xc_pair(int ch, int c, int c0, const float *f, const float *fts, bool gather)
{
    XcPair s;
    s.live = ch < c;
    s.hi_live = ch + 1 < c;
    const int cc = s.live ? ch : (c - 1) & ~1;   // clamped: a valid even channel
    s.hi = s.hi_live ? 1u : 0u;
    s.gathered = gather && cc >= c0;
    s.base = s.gathered ? fts + (cc - c0) : f + cc;
    return s;
}

template <bool V2>
__device__ __forceinline__ f2 ld_pair(const float *p, unsigned hi)
{
    if constexpr (V2) return *reinterpret_cast<const f2 *>(p);
    else return f2{p[0], p[hi]};
}

// the 2 * M floats of a channel pair in a (rows, C * M) tensor: channel ch's M values, then ch + 1's
template <int M, bool V2>
__device__ __forceinline__ void st_pair_m(float *p, bool hi_live, const f2 (&v)[M])
{
    if constexpr (V2) {
#pragma unroll
        for (int q = 0; q < M; ++q) {
            const int e0 = 2 * q, e1 = 2 * q + 1;
            reinterpret_cast<f2 *>(p)[q] = f2{e0 < M ? v[e0].x : v[e0 - M].y, e1 < M ? v[e1].x : v[e1 - M].y};
        }
    } else {
#pragma unroll
        for (int m = 0; m < M; ++m) p[m] = v[m].x;
        if (hi_live) {
#pragma unroll
            for (int m = 0; m < M; ++m) p[M + m] = v[m].y;
        }
    }
}

// Rows of a wave: r0 + wave + 4 i (i = 0, 1, ...), as one wave per row walked them, taken R at a time: the R rows' index
// loads and neighbour gathers are all issued before the first row's products.  A row past the block's end is clamped to the
// last row (its loads stay valid) and not stored.  Table base of a row's cloud: tracked per wave as the rows ascend, no
// division per row.
constexpr int kXcRows = 2;

struct XcCloud {
    long long next;   // first row of the next cloud
    unsigned tbase;   // first table row of the current cloud
};

__device__ __forceinline__ unsigned xc_tbase(XcCloud &cl, long long r, int rows_per_cloud, int n_src)
{
    while (r >= cl.next) { cl.next += rows_per_cloud; cl.tbase += static_cast<unsigned>(n_src); }
    return cl.tbase;
}

// xc_tbase with its loop kept a loop: left visible, the compiler replaces it by the closed form, a 64-bit division per row
__device__ __forceinline__ unsigned xc_tbase_step(XcCloud &cl, long long r, int rows_per_cloud, int n_src)
{
    while (r >= cl.next) {
        cl.next += rows_per_cloud;
        cl.tbase += static_cast<unsigned>(n_src);
        asm volatile("" : "+s"(cl.tbase));
    }
    return cl.tbase;
}

__device__ __forceinline__ XcCloud xc_cloud(long long r, int rows_per_cloud, int n_src)
{
    const long long b = r / rows_per_cloud;
    return XcCloud{(b + 1) * rows_per_cloud, static_cast<unsigned>(b * n_src)};
}

// the K neighbour pairs of row r: lifted rows r K + j (stride cl_stride), gathered rows tbase + idx[r K + j] (stride c1)
template <int K, bool GATHER, bool V2>
__device__ __forceinline__ void xc_gather_row(const XcPair &s, long long r, unsigned tbase, const int *__restrict__ idx,
                                              unsigned lstride, unsigned c1, f2 (&fv)[K])
{
    const unsigned rk = static_cast<unsigned>(r) * K;
#pragma unroll
    for (int j = 0; j < K; ++j) {
        const unsigned lo = (rk + j) * lstride;
        unsigned off = lo;
        if constexpr (GATHER) {
            const unsigned go = (tbase + static_cast<unsigned>(idx[rk + j])) * c1;
            off = s.gathered ? go : lo;
        }
        fv[j] = ld_pair<V2>(s.base + off, s.hi);
    }
}

// X rows of a trip: one coalesced load per 64 coefficients into registers (issued before the gathers), then into the wave's
// LDS slots, from where the products read them as broadcasts.  As scalar operands the packed products need each coefficient
// twice ({x, x} in an SGPR pair): the 64 floats of a row no longer fit and spilled; an LDS broadcast feeds v_pk_mul_f32 with
// op_sel instead.
template <int K>
struct XcXRows {
    static constexpr int KK = K * K, Q = (KK + 63) / 64;
    float v[kXcRows][Q];
    __device__ __forceinline__ void load(const float *__restrict__ x, const long long (&rr)[kXcRows], int lane)
    {
#pragma unroll
        for (int i = 0; i < kXcRows; ++i)
#pragma unroll
            for (int q = 0; q < Q; ++q) {
                const int p = lane + 64 * q;
                v[i][q] = x[rr[i] * KK + (p < KK ? p : KK - 1)];
            }
    }
    __device__ __forceinline__ void stage(float (*xs)[KK], int lane) const
    {
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");   // the previous trip's reads are done
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int i = 0; i < kXcRows; ++i)
#pragma unroll
            for (int q = 0; q < Q; ++q)
                if (lane + 64 * q < KK) xs[i][lane + 64 * q] = v[i][q];
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
};

// Lane-per-channel source of xconv_dw_bwd_fw_kernel (64 channels per block column): c0 is a multiple of 64, so a chunk lies
// on one side of the lifted / gathered split.
struct XcSource {
    const float *base;   // + the lane's channel
    long long stride;
    bool gathered;
};

__device__ __forceinline__ XcSource xc_source(int ch, int c, int c0, const float *f, const float *fts, const int *idx)
{
    XcSource s;
    if (idx == nullptr) { s.base = f + ch; s.stride = c; s.gathered = false; }
    else if (ch - (ch & 63) < c0) { s.base = f + ch; s.stride = c0; s.gathered = false; }
    else { s.base = fts + (ch - c0); s.stride = c - c0; s.gathered = true; }
    return s;
}

// a float at a wave-uniform base plus a 32-bit byte offset per lane: the load takes the base from scalar registers
__device__ __forceinline__ const float *xc_at(const float *base, unsigned byte_off)
{
    return reinterpret_cast<const float *>(reinterpret_cast<const char *>(base) + byte_off);
}

// A wave-uniform row base in global memory, made opaque to the optimiser (two scalar registers pass through an empty asm): left
// visible, the lane's loop-invariant offset is folded into the tensor's base outside the loop, or into a sum shared by the K
// accesses of a row, and every access forms a 64-bit address in vector registers.  Opaque, the access takes its base from the
// scalar pair and the lane's 32-bit offset as it is.
typedef __attribute__((address_space(1))) float xc_gfloat;
__device__ __forceinline__ xc_gfloat *xc_sbase(const float *p)
{
    const unsigned long long b = reinterpret_cast<unsigned long long>(p);
    unsigned lo = __builtin_amdgcn_readfirstlane(static_cast<unsigned>(b)), hi = __builtin_amdgcn_readfirstlane(static_cast<unsigned>(b >> 32));
    asm("" : "+s"(lo), "+s"(hi));
    return (xc_gfloat *)((static_cast<unsigned long long>(hi) << 32) | lo);
}
// a lane's loop-invariant offset as a value of the loop's own (one register move): hoisted out of the loop, its 64-bit extension
// is all the instruction selector sees, and the scalar-base form of the access is not chosen
__device__ __forceinline__ unsigned xc_lane_off(unsigned off)
{
    asm volatile("" : "+v"(off));
    return off;
}
__device__ __forceinline__ xc_gfloat *xc_gat(xc_gfloat *base, unsigned byte_off)
{
    return (xc_gfloat *)((__attribute__((address_space(1))) char *)base + byte_off);
}

// the M floats of a (row, channel) pair at p; `arg` is the tensor's first element (a kernel argument), whose alignment decides
// for every (row, channel) pair alike
template <int M>
__device__ __forceinline__ void xc_load_m(const float *arg, const float *p, float (&v)[M])
{
    if constexpr (M == 4) {
        if ((reinterpret_cast<uintptr_t>(arg) & 15) == 0) {
            const float4 t = *reinterpret_cast<const float4 *>(p);
            v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
            return;
        }
    } else if constexpr (M == 2) {
        if ((reinterpret_cast<uintptr_t>(arg) & 7) == 0) { const float2 t = *reinterpret_cast<const float2 *>(p); v[0] = t.x; v[1] = t.y; return; }
    }
#pragma unroll
    for (int m = 0; m < M; ++m) v[m] = p[m];
}

// xc_load_m through a global-memory pointer
template <int M>
__device__ __forceinline__ void xc_gload_m(const float *arg, xc_gfloat *p, float (&v)[M])
{
    typedef float v4 __attribute__((ext_vector_type(4)));
    if constexpr (M == 4) {
        if ((reinterpret_cast<uintptr_t>(arg) & 15) == 0) {
            const v4 t = *(__attribute__((address_space(1))) v4 *)p;
            v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
            return;
        }
    } else if constexpr (M == 2) {
        if ((reinterpret_cast<uintptr_t>(arg) & 7) == 0) { const f2 t = *(__attribute__((address_space(1))) f2 *)p; v[0] = t.x; v[1] = t.y; return; }
    }
#pragma unroll
    for (int m = 0; m < M; ++m) v[m] = p[m];
}

// A batch of xconv_dw_bwd_fw_kernel: the operands of a wave's R rows as loaded (X still in registers, one coalesced load per 64
// coefficients; the lifted values of the BN twin still un-normalised).
template <int K, int M, int R>
struct XcFwBatch {
    static constexpr int Q = (K * K + 63) / 64;
    float x[R][Q];
    f2 fv[R][K / 2];   // pairs of neighbours: a packed product takes one half as its broadcast operand
    float g[R][M];
};
// Rows of a wave in flight (the batch): kXcRows wherever 128 VGPRs hold them without a spill (four blocks per CU, one wave of each
// per SIMD: see xdw_bwd_grid), else one; see profiles/xconv_instantiations.md and profiles/xconv_bn_instantiations.md.
constexpr int xc_fw_rows(int k, int m, bool bn) { return k * m >= 24 ? 1 : kXcRows; }
// Where the lane's K x M depthwise weights live during the row loop: in registers, or, where those 2 K M registers (weights and
// their gradient sums) leave no room, in the block's reduction buffer, idle until the loop ends, read per pair of k
constexpr bool xc_fw_wd_lds(int k, int m) { return k * m >= 32; }
// Whether the next batch's loads are issued ahead of the current batch's products (a second XcFwBatch in registers)
constexpr bool xc_fw_pipe(int k, int m, bool bn) { return k == 4 || k * m <= 8; }

// ---- the fused kernels: ONE template per pass, instantiated by xconv.hip (BN off, HF_XDW_DISPATCH, both GATHER) and by xconv_bn.hip
// (BN on, GATHER on, HF_XBN_DISPATCH).  `BN` switches the normalisation on load and the dgamma / dbeta sums on: the folded route and
// the two-launch route give the same bits because they run the same code.  A launch with BN off passes null for gamma, beta, mean,
// invstd (and bn_partial).  The forward and the F / Wd gradient are the __global__ templates themselves -- as inlined bodies behind
// per-file wrappers the compiler schedules several instantiations differently (K = 12 takes half as many instructions again) --
// the X gradient is a body (xc_bwd_x_body) behind the two files' wrappers.

// X-transform apply and the depthwise step of the separable convolution in one pass (pointcnn.py:133-140):
//   out[r][ch*M + m] = sum_k (sum_j X[r][k][j] * F[r][j][ch]) * Wd[k][ch][m]
// F_X = X x F_* (rows x K x C, the largest tensor of an X-Conv: 1.3 GB for the decoder layers at 131 072 points) is never
// written: the K products of a (row, channel) stay in registers.  Same multiply / add order as hf_xconv_apply followed by
// hf_depthwise_k, so the results are bit-identical to the two-kernel route.
// Mapping: a lane owns one channel pair for the whole kernel (its K x M depthwise weights live in registers, blockIdx.y picks
// the 128-channel chunk), the four waves of a block walk the rows of a chunk; the row's K x K matrix is wave-uniform.
//
// GATHER: F_* = [F_delta | F gathered] (pointcnn.py:124-127 concat of the lifted coordinates with the neighbours' features) is
// not materialised either: channels below c0 come from `f` = F_delta (rows x K x c0), the others from the feature table
// `fts` (clouds x n_src rows x c - c0) through the neighbour table `idx` (rows x K, indices inside the row's cloud).  The gathered
// rows (K x the table, 1.1 GB for the last decoder layers) were written by group_point and read back here; now the table (134 MB,
// L2 / MALL resident) is read in place.
// BN: `f` is the lifting chain's pre-activation z1 and F_delta = BN1(elu(z1)) is rebuilt on load with bn_apply_kernel's sequence,
// a = gamma * invstd; h = a * (elu_stream(z) - mean) + beta (multiply, then add: -ffp-contract=off).
template <int K, int M, bool GATHER, bool V2, bool BN>
__global__ __launch_bounds__(kXcThreads) void xconv_dw_fwd_kernel(long long rows, int c, int c0, int rows_per_block,
                                                                 const float *__restrict__ x, const float *__restrict__ f,
                                                                 const float *__restrict__ gamma, const float *__restrict__ beta,
                                                                 const float *__restrict__ mean, const float *__restrict__ invstd,
                                                                 const float *__restrict__ fts, const int *__restrict__ idx, int n_src,
                                                                 int rows_per_cloud, const float *__restrict__ wd, float *__restrict__ out)
{
    static_assert(GATHER || !BN, "the BatchNorm fold exists on the gather route only");
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6));
    const int ch = blockIdx.y * 128 + 2 * lane;
    const XcPair src = xc_pair(ch, c, c0, f, fts, GATHER);
    const int cw = src.live ? ch : (c - 1) & ~1;
    f2 w[K][M];
#pragma unroll
    for (int k = 0; k < K; ++k)
#pragma unroll
        for (int m = 0; m < M; ++m) w[k][m] = f2{wd[(static_cast<size_t>(k) * c + cw) * M + m], wd[(static_cast<size_t>(k) * c + cw + src.hi) * M + m]};
    // BN: the pair's BatchNorm constants, loaded once like w (c0 is even: a lifted pair lies below c0 as a whole); a gathered lane
    // reads channel 0's, computes with them and keeps the raw value by select
    bool some_lifted = false;   // this block column holds lifted channels
    f2 ba, bmu, bb;
    if constexpr (BN) {
        const int cb = src.gathered ? 0 : cw;
        some_lifted = static_cast<int>(blockIdx.y) * 128 < c0;
        ba = f2{gamma[cb] * invstd[cb], gamma[cb + 1] * invstd[cb + 1]};
        bmu = f2{mean[cb], mean[cb + 1]};
        bb = f2{beta[cb], beta[cb + 1]};
    }
    const unsigned lstride = GATHER ? c0 : c, c1 = c - c0;
    const long long r0 = static_cast<long long>(blockIdx.x) * rows_per_block;
    const long long r1 = r0 + rows_per_block < rows ? r0 + rows_per_block : rows;
    __shared__ float xs[kXcThreads / 64][kXcRows][K * K];
    XcCloud cl = xc_cloud(r0, rows_per_cloud, n_src);
    for (long long rb = r0 + wave; rb < r1; rb += 4 * kXcRows) {
        f2 fv[kXcRows][K];
        long long rr[kXcRows];
#pragma unroll
        for (int i = 0; i < kXcRows; ++i) rr[i] = rb + 4 * i < r1 ? rb + 4 * i : r1 - 1;
        XcXRows<K> xrow;
        xrow.load(x, rr, lane);
#pragma unroll
        for (int i = 0; i < kXcRows; ++i) {
            const unsigned tb = GATHER ? xc_tbase(cl, rr[i], rows_per_cloud, n_src) : 0u;
            xc_gather_row<K, GATHER, V2>(src, rr[i], tb, idx, lstride, c1, fv[i]);
        }
        xrow.stage(xs[wave], lane);
#pragma unroll
        for (int i = 0; i < kXcRows; ++i) {
            if (rb + 4 * i >= r1) break;
            if constexpr (BN) {
                if (some_lifted) {   // uniform over the block: the columns past the split (most of them) pay nothing
#pragma unroll
                    for (int j = 0; j < K; ++j) {
                        const f2 z = fv[i][j];
                        const f2 h = ba * (f2{elu_stream(z.x), elu_stream(z.y)} - bmu) + bb;
                        fv[i][j] = src.gathered ? z : h;
                    }
                }
            }
            const float *xr = xs[wave][i];
            f2 o[M];
#pragma unroll
            for (int m = 0; m < M; ++m) o[m] = f2{0.f, 0.f};
#pragma unroll
            for (int k = 0; k < K; ++k) {
                f2 t = xr[k * K] * fv[i][0];
#pragma unroll
                for (int j = 1; j < K; ++j) t = t + xr[k * K + j] * fv[i][j];
#pragma unroll
                for (int m = 0; m < M; ++m) o[m] = o[m] + t * w[k][m];
            }
            if (src.live) st_pair_m<M, V2>(out + static_cast<size_t>(rr[i] * c + ch) * M, src.hi_live, o);
        }
    }
}

// gradients w.r.t. F and Wd: a lane owns ONE channel (64 per block column, see XcSource); per (row, channel) the gradient of F_X
// (K values), F_X itself (recomputed) and the K input gradients stay in registers; a lane sums its channel's K x M weight gradients
// over its rows.
// GATHER: grad_f is the gradient of F_delta only (rows x K x c0); the gathered channels' gradient is either written to
// grad_gathered (rows x K x c1, then summed per table row by hf_group_point_grad_gather) or rebuilt per table row by
// xconv_dw_bwd_fts_kernel.
// BN: the lifted values are normalised on load, and the two BatchNorm-backward sums of the lifted channels (bn_bwd_reduce_kernel's
// expressions on the gradient this kernel stores) are formed on the way: a lane owns one channel over all its rows, as it does for
// the Wd gradient; the four waves meet in LDS in wave order and the block writes bn_partial[blockIdx.x][0][c0] = sum gf,
// bn_partial[blockIdx.x][1][c0] = sum gf * xhat (xconv_bn_finalize_kernel adds the blocks).  wd_partial is always there: no atomics.
// The row loop: wave w of a block takes rows r0 + w + 4 i in ascending order, R of them per batch (xc_fw_rows).  Every load of a batch
// -- the neighbour indices (scalar, read one batch ahead), the R rows' X (one coalesced load per 64 coefficients), K neighbour
// values and grad_out -- is issued before the first row's products, through wave-uniform 64-bit row bases with 32-bit lane offsets;
// where the registers allow (xc_fw_pipe) the NEXT batch's loads are issued before the current batch's products.  A row past the
// block's end is clamped to the last row (its loads stay valid) and skipped; a lane past the last channel reads the last channel
// and stores nothing.  X goes from the registers into the wave's own LDS slot and is read back as broadcasts: as scalar operands
// the 64 coefficients of a row and the 17 pointer arguments did not fit the scalar file, and about 80 lane moves per row carried
// the spills.  The products run packed on pairs of k (F_X, dF_X, the weight gradient) and pairs of j (the input gradient); every
// output element keeps the sequence of multiplies and adds it had, so the results are the bits of the one-row-at-a-time form.
// amdgpu_waves_per_eu(4): the grid is four blocks per CU (xdw_bwd_grid), one wave of each per SIMD, so 128 VGPRs; nothing spills
// (profiles/xconv_instantiations.md, profiles/xconv_bn_instantiations.md).
template <int K, int M, bool GATHER, bool BN>
__global__ __launch_bounds__(kXcThreads) __attribute__((amdgpu_waves_per_eu(4))) void xconv_dw_bwd_fw_kernel(
    long long rows, int c, int c0, int rows_per_block, const float *__restrict__ x, const float *__restrict__ f,
    const float *__restrict__ gamma, const float *__restrict__ beta, const float *__restrict__ mean, const float *__restrict__ invstd,
    const float *__restrict__ fts, const int *__restrict__ idx, int n_src, int rows_per_cloud, const float *__restrict__ wd,
    const float *__restrict__ grad_out, float *__restrict__ grad_f, float *__restrict__ grad_gathered, float *__restrict__ grad_wd,
    float *__restrict__ wd_partial, float *__restrict__ bn_partial)
{
    static_assert(GATHER || !BN, "the BatchNorm fold exists on the gather route only");
    constexpr int R = xc_fw_rows(K, M, BN), Q = XcFwBatch<K, M, R>::Q;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6));
    const int ch = blockIdx.y * 64 + lane;
    const bool live = ch < c;
    const XcSource src = xc_source(live ? ch : blockIdx.y * 64, c, c0, f, fts, GATHER ? idx : nullptr);
    if (GATHER && src.gathered && !grad_wd && !grad_gathered) return;   // nothing of this chunk is asked for (no partial to write either)
    bool lifted = false;   // BN: = !src.gathered, uniform over the block; every lane of a lifted chunk is live
    float bis, ba, bmu, bb, s1 = 0.f, s2 = 0.f;
    if constexpr (BN) {
        lifted = static_cast<int>(blockIdx.y) * 64 < c0;
        const int cb = lifted ? ch : 0;
        bis = invstd[cb]; ba = gamma[cb] * bis; bmu = mean[cb]; bb = beta[cb];
    }
    // Packed f32 across PAIRS OF k: the lane keeps its single channel, and {k, k + 1} values of dF_X, F_X and the weight gradient go
    // through v_pk_mul_f32 / v_pk_add_f32 (each half rounds like the scalar op; every element keeps its own multiply / add sequence).
    static_assert(K % 2 == 0, "pairs of k");
    constexpr bool WL = xc_fw_wd_lds(K, M);
    __shared__ float red[K * M][64];
    f2 *const wl = reinterpret_cast<f2 *>(&red[0][0]) + lane * M;   // WL: [pair of k][lane][m], the same 64 channels for the four waves
    f2 w[WL ? 1 : K / 2][M], gw[K / 2][M];
#pragma unroll
    for (int kp = 0; kp < K / 2; ++kp)
#pragma unroll
        for (int m = 0; m < M; ++m) {
            const f2 wk = live ? f2{wd[(static_cast<size_t>(2 * kp) * c + ch) * M + m], wd[(static_cast<size_t>(2 * kp + 1) * c + ch) * M + m]} : f2{0.f, 0.f};
            if constexpr (WL) { if (wave == 0) wl[kp * 64 * M + m] = wk; }
            else w[kp][m] = wk;
            gw[kp][m] = f2{0.f, 0.f};
        }
    if constexpr (WL) __syncthreads();
    const long long r0 = static_cast<long long>(blockIdx.x) * rows_per_block;
    const long long r1 = r0 + rows_per_block < rows ? r0 + rows_per_block : rows;
    // what a lane adds to the wave-uniform row bases: its channel inside the source's row (a dead lane reads the last channel, which
    // lies in its chunk, and stores nothing), and its M floats of grad_out
    const bool gathered = GATHER && static_cast<int>(blockIdx.y) * 64 >= c0;   // = src.gathered, from scalars alone
    const int cc = live ? ch : c - 1;
    const unsigned stride = static_cast<unsigned>(GATHER ? (gathered ? c - c0 : c0) : c);   // = src.stride
    const unsigned foff = static_cast<unsigned>(gathered ? cc - c0 : cc) * 4u, goff = static_cast<unsigned>(cc) * (4u * M);
    unsigned xoff[Q];   // the lane's coefficients of a row's X: one coalesced load per 64
#pragma unroll
    for (int q = 0; q < Q; ++q) xoff[q] = static_cast<unsigned>(lane + 64 * q < K * K ? lane + 64 * q : K * K - 1) * 4u;
    float *const gdst = gathered ? grad_gathered : grad_f;   // wave-uniform: where the K input gradients of a (row, channel) go, if asked for
    // a row's X in the wave's own LDS slot, twice: [0] with the matrix rows of a pair interleaved ({X[k][j], X[k + 1][j]} adjacent, for
    // F_X on pairs of k) and [1] as it is ({X[k][j], X[k][j + 1]}, for the transposed product on pairs of j); both are read as broadcasts
    __shared__ float xs[kXcThreads / 64][R][2][K * K];
    unsigned xpos[Q];   // where the lane's coefficient goes in the interleaved copy
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        const int e = lane + 64 * q < K * K ? lane + 64 * q : K * K - 1, k = e / K, j = e - k * K;
        xpos[q] = ((k >> 1) * K + j) * 2 + (k & 1);
    }
    auto stage = [&](const float (&xr)[R][Q]) {
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");   // the previous batch's reads are done
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int i = 0; i < R; ++i)
#pragma unroll
            for (int q = 0; q < Q; ++q)
                if (lane + 64 * q < K * K) { xs[wave][i][0][xpos[q]] = xr[i][q]; xs[wave][i][1][lane + 64 * q] = xr[i][q]; }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        __builtin_amdgcn_wave_barrier();
    };
    XcCloud cl = xc_cloud(r0, rows_per_cloud, n_src);
    constexpr bool PIPE = xc_fw_pipe(K, M, BN);
    XcFwBatch<K, M, R> cur, nxt;
    int nidx[R][K];   // the neighbour indices of the batch whose loads are issued next (wave-uniform)
    auto clamp_rows = [&](long long rb, long long (&rr)[R]) {
#pragma unroll
        for (int i = 0; i < R; ++i) rr[i] = rb + 4 * i < r1 ? rb + 4 * i : r1 - 1;
    };
    auto load_idx = [&](long long rb) __attribute__((always_inline)) {
        if (gathered) {
            long long rr[R];
            clamp_rows(rb, rr);
#pragma unroll
            for (int i = 0; i < R; ++i)
#pragma unroll
                for (int j = 0; j < K; ++j) nidx[i][j] = idx[rr[i] * K + j];
        }
    };
    auto issue = [&](long long rb, XcFwBatch<K, M, R> &o) __attribute__((always_inline)) {   // every load of a batch, from nidx = its rows' indices
        long long rr[R];
        clamp_rows(rb, rr);
#pragma unroll
        for (int i = 0; i < R; ++i) {
            xc_gfloat *xb = xc_sbase(x + rr[i] * (K * K));
#pragma unroll
            for (int q = 0; q < Q; ++q) o.x[i][q] = *xc_gat(xb, xc_lane_off(xoff[q]));
        }
#pragma unroll
        for (int i = 0; i < R; ++i) {
            const unsigned fo = xc_lane_off(foff);
            if (gathered) {
                const unsigned tb = xc_tbase_step(cl, rr[i], rows_per_cloud, n_src);
#pragma unroll
                for (int j = 0; j < K; ++j)
                    o.fv[i][j / 2][j % 2] = *xc_gat(xc_sbase(fts + static_cast<unsigned long long>(tb + static_cast<unsigned>(nidx[i][j])) * stride), fo);
            } else {
                const float *fl = f + rr[i] * K * static_cast<long long>(stride);
#pragma unroll
                for (int j = 0; j < K; ++j) o.fv[i][j / 2][j % 2] = *xc_gat(xc_sbase(fl + j * static_cast<size_t>(stride)), fo);
            }
            xc_gload_m<M>(grad_out, xc_gat(xc_sbase(grad_out + rr[i] * c * static_cast<long long>(M)), xc_lane_off(goff)), o.g[i]);
        }
    };
    // one row's products, a pair of k at a time: dF_X[k], F_X[k] (from the interleaved copy of X) and the weight gradient, and, with
    // GA, the two terms k, k + 1 of the K input gradients (from the plain copy): ga[j] takes its terms in ascending k
    auto row = [&](auto ga_tag, const float *xr, long long r, const f2 (&fin)[K / 2], const float (&g)[M]) {
        constexpr bool GA = decltype(ga_tag)::value;
        f2 fv[K / 2], xv[K / 2];
        float ga[K];
#pragma unroll
        for (int j = 0; j < K / 2; ++j) fv[j] = fin[j];
        if constexpr (BN) {
            if (lifted) {   // z1 -> F_delta, elu(z1) kept for the sums below
#pragma unroll
                for (int j = 0; j < K / 2; ++j) {
                    xv[j] = f2{elu_stream(fv[j].x), elu_stream(fv[j].y)};
                    fv[j] = ba * (xv[j] - bmu) + bb;
                }
            }
        }
        const f2 *xp = reinterpret_cast<const f2 *>(xr), *xn = reinterpret_cast<const f2 *>(xr + K * K);
        f2 gap[K / 2];
#pragma unroll
        for (int kp = 0; kp < K / 2; ++kp) {
            f2 a = f2{0.f, 0.f};
#pragma unroll
            for (int m = 0; m < M; ++m) a = a + g[m] * (WL ? wl[kp * 64 * M + m] : w[WL ? 0 : kp][m]);   // = hf_depthwise_k_grad's dx
            f2 t = xp[kp * K] * fv[0].x;                                      // F_X recomputed
#pragma unroll
            for (int j = 1; j < K; ++j) t = t + xp[kp * K + j] * fv[j / 2][j % 2];
#pragma unroll
            for (int m = 0; m < M; ++m) {
                gw[kp][m] = gw[kp][m] + t * g[m];                             // = hf_depthwise_k_grad's dw
                asm volatile("" : "+v"(gw[kp][m]));   // here, not behind the stores below, where the compiler moves it with all of X live
            }
            if constexpr (GA) {   // = hf_xconv_apply_grad's dF (X transposed): ga[j] takes its K terms in ascending k
#pragma unroll
                for (int jp = 0; jp < K / 2; ++jp) gap[jp] = kp == 0 ? xn[jp] * a.x : gap[jp] + xn[2 * kp * (K / 2) + jp] * a.x;
#pragma unroll
                for (int jp = 0; jp < K / 2; ++jp) gap[jp] = gap[jp] + xn[(2 * kp + 1) * (K / 2) + jp] * a.y;
            }
            __builtin_amdgcn_sched_barrier(0);   // a pair of k at a time: left free, the scheduler reads all of X ahead (64 registers)
        }
        if constexpr (GA) {
#pragma unroll
            for (int jp = 0; jp < K / 2; ++jp) { ga[2 * jp] = gap[jp].x; ga[2 * jp + 1] = gap[jp].y; }
            float *gd = gdst + r * K * static_cast<long long>(stride);
            // ga is complete here in every lane: left to the compiler, the K x K products move behind `live` and with them all of X
#pragma unroll
            for (int j = 0; j < K; ++j) asm volatile("" : "+v"(ga[j]));
            const unsigned fo = xc_lane_off(foff);
            if (live) {
#pragma unroll
                for (int j = 0; j < K; ++j) *xc_gat(xc_sbase(gd + j * static_cast<size_t>(stride)), fo) = ga[j];
            }
            if constexpr (BN) {
                if (lifted) {   // = bn_bwd_reduce_kernel's sums with dh = the value just stored
#pragma unroll
                    for (int j = 0; j < K; ++j) { s1 += ga[j]; s2 += ga[j] * ((xv[j / 2][j % 2] - bmu) * bis); }
                }
            }
        }
    };
    // the row loop, once with the K input gradients and once without: the choice (wave-uniform) is made here, outside the loop, so
    // that each form keeps its own schedule
    auto run = [&](auto ga_tag) __attribute__((always_inline)) {
        const long long rb0 = r0 + wave;
        if (rb0 < r1) {
            load_idx(rb0);
            if constexpr (PIPE) {
                issue(rb0, cur);
                load_idx(rb0 + 4 * R);
            }
        }
        for (long long rb = rb0; rb < r1; rb += 4 * R) {
            if constexpr (PIPE) {   // the next batch's loads ahead of this batch's products (past the end: the last row again, dropped)
                issue(rb + 4 * R, nxt);
                load_idx(rb + 8 * R);
            } else {
                issue(rb, cur);
                load_idx(rb + 4 * R);
            }
            stage(cur.x);
#pragma unroll
            for (int i = 0; i < R; ++i) {
                if (rb + 4 * i >= r1) break;
                row(ga_tag, xs[wave][i][0], rb + 4 * i, cur.fv[i], cur.g[i]);
            }
            if constexpr (PIPE) cur = nxt;
        }
    };
    if (gdst) run(std::true_type{});
    else run(std::false_type{});
    if constexpr (WL) __syncthreads();   // every wave is done with the weights in `red`
    if constexpr (BN) {
        if (lifted && grad_f) {
            // the waves take turns, wave 0 first, on two rows of `red` (a fixed order of adds); the Wd reduction below reuses them
            for (int wv = 0; wv < kXcThreads / 64; ++wv) {
                if (wave == wv) {
                    red[0][lane] = wv == 0 ? s1 : red[0][lane] + s1;
                    red[1][lane] = wv == 0 ? s2 : red[1][lane] + s2;
                }
                __syncthreads();
            }
            if (wave == 0) {   // the slots it reads are its own: the first writer below is this same thread
                float *mine = bn_partial + static_cast<size_t>(blockIdx.x) * 2 * c0;
                mine[ch] = red[0][lane];
                mine[c0 + ch] = red[1][lane];
            }
        }
    }
    if (grad_wd) {
        // the waves of a block meet in LDS first: one sum per coefficient and BLOCK (per wave it was 8.4 M atomics on 2080 addresses
        // for the first encoder layer: 870 us for 140 us of memory traffic)
        // The waves take turns, wave 0 first: a fixed order of adds (LDS atomics left it to the order the waves arrived in), so with
        // wd_partial grad_wd is the same bits on every call.  The slots of dead lanes are neither written nor read.
        for (int wv = 0; wv < kXcThreads / 64; ++wv) {
            if (wave == wv && live) {
#pragma unroll
                for (int k = 0; k < K; ++k)
#pragma unroll
                    for (int m = 0; m < M; ++m) red[k * M + m][lane] = wv == 0 ? gw[k / 2][m][k % 2] : red[k * M + m][lane] + gw[k / 2][m][k % 2];
            }
            __syncthreads();
        }
        // wd_partial (always with BN): the row chunks' sums are written out (wd_partial[row chunk][K*c*M]) and added in a fixed order
        // by a second kernel; else one global atomic per coefficient and block on grad_wd (zero-filled by the entry point)
        float *mine = (BN || wd_partial) ? wd_partial + static_cast<size_t>(blockIdx.x) * K * c * M : nullptr;
        for (int i = threadIdx.x; i < K * M * 64; i += kXcThreads) {
            const int km = i >> 6, c2 = blockIdx.y * 64 + (i & 63);
            if (c2 < c) {
                const size_t e = (static_cast<size_t>(km / M) * c + c2) * M + km % M;
                if (BN || mine) mine[e] = red[km][i & 63];
                else atomicAdd(&grad_wd[e], red[km][i & 63]);
            }
        }
    }
}

// ---- the X gradient: xconv_dw_bwd_x_kernel / xconv_bn_bwd_x_kernel ----
// Addresses: a row's tensors are reached through wave-uniform 64-bit bases (F + r K stride, grad_out + r c M, the K table rows of
// the row's neighbours) formed on the scalar side once per row; a lane adds a 32-bit element offset (its channel, plus j * stride
// inside the row's K x stride block of F), so the loads take their base from scalar registers and no 64-bit product is formed
// per element.  The offset inside a row is below K c M, whatever the tensor's size: nothing here depends on xdw_offsets_fit.

// first table row of row r's cloud; `next` is the first row of the following cloud.  The division runs only when a wave's rows
// cross into another cloud (rows ascend per wave, by any stride).
struct XcCloudDiv {
    long long first, next;
    long long tbase;
};

__device__ __forceinline__ long long xc_tbase_div(XcCloudDiv &cl, long long r, int rows_per_cloud, int n_src)
{
    if (r >= cl.next || r < cl.first) {
        const long long b = static_cast<long long>(static_cast<unsigned>(r) / static_cast<unsigned>(rows_per_cloud));
        cl.first = b * rows_per_cloud;
        cl.next = cl.first + rows_per_cloud;
        cl.tbase = b * n_src;
    }
    return cl.tbase;
}

template <int CTRL>
__device__ __forceinline__ float xc_dpp(float v)
{
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, true));
}

// Sum over the 64 lanes of N per-lane values v[OFF .. OFF + N), N = 64 or 16, by halving: in each step a lane hands half of its
// values to a partner lane and adds the partner's other half to the half it keeps, so after log2(N) steps it holds ONE entry.
//   N = 64: six steps; lane l ends with entry OFF + l summed over all 64 lanes, in v[OFF]
//   N = 16: four steps leave entry OFF + (l >> 2) summed over 16 lanes; two adds across the quad finish it (the four lanes of a
//           quad hold the same bits)
// Partners: lane ^ 32 and lane ^ 16 by v_permlane32_swap / v_permlane16_swap (one swap and one add per pair of values, no select),
// lane ^ 8 (row_ror:8), lane ^ 7 (row_half_mirror: the lanes of an 8-group pair up as 0-7, 1-6, 2-5, 3-4; the kept half goes by
// bit 2), lane ^ 2 and lane ^ 1 (quad_perm) by DPP on the add, the half to keep picked by select.  A fixed tree: 6 adds on every
// path, no LDS, no atomics, the same bits on every call.  63 (N = 64) / 17 (N = 16) adds per lane in all.
template <int KK, int OFF, int N>
__device__ __forceinline__ void xc_lane_fold(float (&v)[KK], int lane)
{
    static_assert(N == 64 || N == 16, "chunks of 64 or 16 entries");
    typedef unsigned u2 __attribute__((ext_vector_type(2)));
#pragma unroll
    for (int i = 0; i < N / 2; ++i) {
        const u2 s = __builtin_amdgcn_permlane32_swap(__float_as_uint(v[OFF + i]), __float_as_uint(v[OFF + i + N / 2]), false, false);
        v[OFF + i] = __uint_as_float(s.x) + __uint_as_float(s.y);
    }
#pragma unroll
    for (int i = 0; i < N / 4; ++i) {
        const u2 s = __builtin_amdgcn_permlane16_swap(__float_as_uint(v[OFF + i]), __float_as_uint(v[OFF + i + N / 4]), false, false);
        v[OFF + i] = __uint_as_float(s.x) + __uint_as_float(s.y);
    }
    const bool b3 = (lane & 8) != 0, b2 = (lane & 4) != 0;
#pragma unroll
    for (int i = 0; i < N / 8; ++i) {
        const float lo = v[OFF + i], hi = v[OFF + i + N / 8];
        v[OFF + i] = (b3 ? hi : lo) + xc_dpp<0x128>(b3 ? lo : hi);
    }
#pragma unroll
    for (int i = 0; i < N / 16; ++i) {
        const float lo = v[OFF + i], hi = v[OFF + i + N / 16];
        v[OFF + i] = (b2 ? hi : lo) + xc_dpp<0x141>(b2 ? lo : hi);
    }
    if constexpr (N == 64) {
        const bool b1 = (lane & 2) != 0, b0 = (lane & 1) != 0;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const float lo = v[OFF + i], hi = v[OFF + i + 2];
            v[OFF + i] = (b1 ? hi : lo) + xc_dpp<0x4e>(b1 ? lo : hi);   // quad_perm [2,3,0,1]
        }
        const float lo = v[OFF], hi = v[OFF + 1];
        v[OFF] = (b0 ? hi : lo) + xc_dpp<0xb1>(b0 ? lo : hi);          // quad_perm [1,0,3,2]
    } else {
        v[OFF] = v[OFF] + xc_dpp<0x4e>(v[OFF]);
        v[OFF] = v[OFF] + xc_dpp<0xb1>(v[OFF]);
    }
}

// the K x K matrix of a row: every 64-entry chunk, then the 16-entry rest (K * K = 16, 64, 144)
template <int KK, int OFF = 0>
__device__ __forceinline__ void xc_store_dx(float (&acc)[KK], int lane, float *__restrict__ dst)
{
    static_assert((KK - OFF) % 64 == 0 || (KK - OFF) % 64 == 16, "K * K is a multiple of 64, or 16 more");
    if constexpr (KK - OFF >= 64) {
        xc_lane_fold<KK, OFF, 64>(acc, lane);
        dst[OFF + lane] = acc[OFF];
        xc_store_dx<KK, OFF + 64>(acc, lane, dst);
    } else if constexpr (KK - OFF == 16) {
        xc_lane_fold<KK, OFF, 16>(acc, lane);
        if ((lane & 3) == 0) dst[OFF + (lane >> 2)] = acc[OFF];
    }
}

// LDS of xconv_*_bwd_x_kernel.  The block's K c M coefficients of Wd are staged once, as [trip][k M + m][64 lanes]: a trip reads its
// K M values at compile-time offsets from one address per lane.  The BN twin stages gamma * invstd, mean and beta of its c0 lifted
// channels behind them (c0 < c: at most 12 KB more).  Staged ("fast") while ceil(c / 64) K M <= kXcWdSlots (16 KB: every shipped
// layer -- dec5 takes 40 slots, enc0 64; K = 8, M = 1 up to c = 512); past it the kernel reads the coefficients and the BatchNorm
// constants from memory in every trip, as it did.
constexpr int kXcWdSlots = 64;
inline __host__ __device__ bool xc_bwd_x_fast(int c, int km) { return ((c + 63) >> 6) * km <= kXcWdSlots; }
inline size_t xc_bwd_x_lds_bytes(int c, int c0_bn, int km)
{
    return xc_bwd_x_fast(c, km) ? sizeof(float) * (64 * static_cast<size_t>((c + 63) >> 6) * km + 3 * static_cast<size_t>(c0_bn)) : 0;
}

// One 64-channel trip's operands of a row, as loaded (the lifted values of the BN twin still un-normalised)
template <int K, int M>
struct XcTrip {
    float fv[K], g[M];
};

// gradient w.r.t. X: dX[r][k][j] = sum_ch dF_X[r][k][ch] * F[r][j][ch], dF_X rebuilt from grad_out and Wd on the fly.
// A wave per row (r = wave, wave + nwaves, ...), lanes walk the channels 64 at a time (a trip).  c0 is a multiple of 64 on the gather
// entries, so a trip lies on one side of the lifted / gathered split: which side is decided once per trip on the scalar side.
// The (row, trip) items of a wave run as one sequence: the next item's loads (the next trip's, or the next row's first trip's) are
// issued before the current item's products -- always, in straight-line code, so that the wait counters stay exact: behind the
// last item they fetch a valid row again and the values are dropped -- and the next row's neighbour indices are read at the
// current row's first trip.
// The accumulators start from the first trip's products (no zero fill; a lane with no channel in the first trip, c < 64, starts
// from 0).  A lane past the last channel loads a clamped, valid channel and skips the products.
// Rounding of an entry: M - 1 adds for dF_X, ceil(c / 64) - 1 across the trips, 6 across the lanes.
template <int K, int M, bool GATHER, bool BN, bool FAST>
__device__ __forceinline__ void xc_bwd_x_rows(long long rows, int c, int c0, const float *__restrict__ f,
                                              const float *__restrict__ gamma, const float *__restrict__ beta,
                                              const float *__restrict__ mean, const float *__restrict__ invstd,
                                              const float *__restrict__ fts, const int *__restrict__ idx, int n_src, int rows_per_cloud,
                                              const float *__restrict__ wd, const float *__restrict__ grad_out,
                                              float *__restrict__ grad_x, float *lds)
{
    constexpr int KK = K * K, KM = K * M;
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6));
    const long long wave = w + static_cast<long long>(blockIdx.x) * (kXcThreads / 64);
    const long long nwaves = static_cast<long long>(gridDim.x) * (kXcThreads / 64);
    const int trips = (c + 63) >> 6, c1 = c - c0;
    const unsigned lstride = GATHER ? c0 : c;
    float *bnl = lds + trips * KM * 64;   // [3][c0]
    if constexpr (FAST) {
        for (int i = threadIdx.x; i < trips * KM * 64; i += kXcThreads) {
            const int l = i & 63, s = i >> 6, t = s / KM, km = s - t * KM, ch = 64 * t + l;
            lds[i] = ch < c ? wd[(static_cast<size_t>(km / M) * c + ch) * M + km % M] : 0.f;
        }
        if constexpr (BN) {
            for (int i = threadIdx.x; i < c0; i += kXcThreads) {
                bnl[i] = gamma[i] * invstd[i];
                bnl[c0 + i] = mean[i];
                bnl[2 * c0 + i] = beta[i];
            }
        }
        __syncthreads();
    }
    if (wave >= rows) return;

    int nidx[K];   // the neighbour indices of the wave's next row (wave-uniform)
    auto load_idx = [&](long long r) {
        if constexpr (GATHER) {
            const long long rc = r < rows ? r : rows - 1;
#pragma unroll
            for (int j = 0; j < K; ++j) nidx[j] = idx[rc * K + j];
        }
    };
    // what addresses a row, formed on the scalar side once per row (from nidx = the row's indices)
    XcCloudDiv cl{0, 0, 0};
    const float *fl = f, *go = grad_out, *tj[K];
    auto set_row = [&](long long r) {
        fl = f + r * K * static_cast<long long>(lstride);
        go = grad_out + r * c * static_cast<long long>(M);
        if constexpr (GATHER) {
            const long long tb = xc_tbase_div(cl, r, rows_per_cloud, n_src);
#pragma unroll
            for (int j = 0; j < K; ++j) tj[j] = fts + static_cast<unsigned long long>(tb + nidx[j]) * static_cast<unsigned>(c1);
        }
    };
    auto load_trip = [&](int t, XcTrip<K, M> &o) {
        const int ch = 64 * t + lane;
        const unsigned cc = ch < c ? ch : c - 1;
        const float *bj[K];
        unsigned sub = 0;
        if (GATHER && 64 * t >= c0) {
            sub = c0;
#pragma unroll
            for (int j = 0; j < K; ++j) bj[j] = tj[j];
        } else {
#pragma unroll
            for (int j = 0; j < K; ++j) bj[j] = fl + j * static_cast<size_t>(lstride);
        }
        const unsigned off = (cc - sub) * 4u;
#pragma unroll
        for (int j = 0; j < K; ++j) o.fv[j] = *xc_at(bj[j], off);
        xc_load_m<M>(grad_out, xc_at(go, cc * (4u * M)), o.g);
    };

    long long r = wave;
    int t = 0;
    load_idx(r);
    set_row(r);
    XcTrip<K, M> cur, nxt;
    load_trip(0, cur);
    static_assert(K % 2 == 0, "pairs of j");
    f2 acc[K][K / 2];
    for (;;) {
        const bool last = t + 1 == trips;
        const long long rn = last ? r + nwaves : r;
        const int tn = last ? 0 : t + 1;
        const bool more = rn < rows;
        if (t == 0) load_idx(r + nwaves);
        if (last) set_row(more ? rn : r);
        load_trip(tn, nxt);
        const int ch = 64 * t + lane;
        const bool live = ch < c;
        const unsigned cc = live ? ch : c - 1;
        if (BN && 64 * t < c0) {   // z1 -> F_delta on the lifted trips
            float ba, bmu, bb;
            if constexpr (FAST) { ba = bnl[cc]; bmu = bnl[c0 + cc]; bb = bnl[2 * c0 + cc]; }
            else { ba = gamma[cc] * invstd[cc]; bmu = mean[cc]; bb = beta[cc]; }
#pragma unroll
            for (int j = 0; j < K; ++j) cur.fv[j] = ba * (elu_stream(cur.fv[j]) - bmu) + bb;
        }
        // dF_X[k] = sum_m g[m] Wd[k][ch][m], on pairs of k (a packed product picks its half below, and no register of a pair
        // belongs to a load still in flight)
        f2 ap[K / 2];
        {
            const float *wt = lds + (t * KM * 64 + lane);
            auto wv = [&](int k, int m) { return FAST ? wt[(k * M + m) * 64] : wd[(static_cast<size_t>(k) * c + cc) * M + m]; };
#pragma unroll
            for (int i = 0; i < K / 2; ++i) {
                ap[i] = cur.g[0] * f2{wv(2 * i, 0), wv(2 * i + 1, 0)};
#pragma unroll
                for (int m = 1; m < M; ++m) ap[i] = ap[i] + cur.g[m] * f2{wv(2 * i, m), wv(2 * i + 1, m)};
            }
        }
        // acc[k][j] (+)= a[k] * fv[j] on pairs of j: the K / 2 packed products of a row of the matrix, then its K / 2 packed adds, so
        // that no add waits on the product issued just before it
        f2 fp[K / 2];
#pragma unroll
        for (int i = 0; i < K / 2; ++i) fp[i] = f2{cur.fv[2 * i], cur.fv[2 * i + 1]};
        if (t == 0) {
            if (live) {
#pragma unroll
                for (int k = 0; k < K; ++k)
#pragma unroll
                    for (int i = 0; i < K / 2; ++i) acc[k][i] = ap[k / 2][k % 2] * fp[i];
            } else {
#pragma unroll
                for (int k = 0; k < K; ++k)
#pragma unroll
                    for (int i = 0; i < K / 2; ++i) acc[k][i] = f2{0.f, 0.f};
            }
        } else if (live) {
#pragma unroll
            for (int k = 0; k < K; ++k) {
                f2 p[K / 2];
#pragma unroll
                for (int i = 0; i < K / 2; ++i) p[i] = ap[k / 2][k % 2] * fp[i];
                __builtin_amdgcn_sched_barrier(0);   // keep the row's products ahead of its adds
#pragma unroll
                for (int i = 0; i < K / 2; ++i) acc[k][i] = acc[k][i] + p[i];
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        if (last) {
            float flat[KK];
#pragma unroll
            for (int k = 0; k < K; ++k)
#pragma unroll
                for (int i = 0; i < K / 2; ++i) { flat[k * K + 2 * i] = acc[k][i].x; flat[k * K + 2 * i + 1] = acc[k][i].y; }
            xc_store_dx<KK>(flat, lane, grad_x + r * KK);
        }
        if (!more) break;
        cur = nxt;
        r = rn;
        t = tn;
    }
}

// the body of xconv_dw_bwd_x_kernel (BN off) and xconv_bn_bwd_x_kernel (BN on): one wave-uniform switch between the staged form
// and the one that reads Wd (and the BatchNorm constants) from memory, no further instantiation of the kernels
template <int K, int M, bool GATHER, bool BN>
__device__ __forceinline__ void xc_bwd_x_body(long long rows, int c, int c0, const float *__restrict__ f,
                                              const float *__restrict__ gamma, const float *__restrict__ beta,
                                              const float *__restrict__ mean, const float *__restrict__ invstd,
                                              const float *__restrict__ fts, const int *__restrict__ idx, int n_src, int rows_per_cloud,
                                              const float *__restrict__ wd, const float *__restrict__ grad_out,
                                              float *__restrict__ grad_x, float *lds)
{
    if (xc_bwd_x_fast(c, K * M))
        xc_bwd_x_rows<K, M, GATHER, BN, true>(rows, c, c0, f, gamma, beta, mean, invstd, fts, idx, n_src, rows_per_cloud, wd, grad_out, grad_x, lds);
    else
        xc_bwd_x_rows<K, M, GATHER, BN, false>(rows, c, c0, f, gamma, beta, mean, invstd, fts, idx, n_src, rows_per_cloud, wd, grad_out, grad_x, lds);
}

// ---- host side, defined in xconv.hip: the launch geometry of the fused kernels and the launcher of the table gradient ----
// forward: channel pairs, 128 channels per block column, ~blocks_per_cu blocks per CU
void xdw_pair_grid(long long rows, int c, dim3 &grid, int &rpb, int blocks_per_cu);
// xconv_dw_bwd_fw_kernel: 64 channels per block column, 4 blocks per CU, at least 32 rows per block
void xdw_bwd_grid(long long rows, int c, dim3 &grid, int &rpb);
// the 32-bit element offsets of the forward kernel reach every element of F (rows x k x c) and of the feature table
bool xdw_offsets_fit(long long rows, int k, int c, long long src_rows);
// channel pairs as 8-byte accesses: c even and every tensor 8-byte aligned
bool xdw_v2(int c, std::initializer_list<const void *> ptrs);
// which route builds the feature table's gradient when a workspace is given (true: rebuilt per table row)
bool xdw_fts_direct(long long rows, int n_src, int rows_per_cloud, int k, int c1, int m);
// bytes of the staging region for the gathered block's gradient at the head of the workspace
size_t xdw_gathered_bytes(int b, int rows_per_cloud, int k, int c1);
// xconv_dw_bwd_fts_kernel: the table's gradient rebuilt per table row from grad_out
int xdw_table_grad(long long src_rows, int n_src, int rows_per_cloud, int k, int c, int c0, int m, const float *x, const float *wd,
                   const float *grad_out, const int *offsets, const int *entries, float *grad_fts, hipStream_t st);

// What hf_xconv_depthwise_gather_grad and hf_xconv_depthwise_gather_bn_grad decide alike once rows > 0 (each keeps its argument
// checks and its launches).  The table's gradient is rebuilt per table row from grad_out (xdw_table_grad: nothing but the table is
// written), or, where xdw_fts_direct says so and a workspace is there, staged: xconv_dw_bwd_fw_kernel writes the gathered block's
// gradient (rows x k x c1) into the workspace and hf_group_point_grad_gather sums it per table row.  The partial weight gradients
// go through the workspace on both routes.
struct XdwGradPlan {
    bool direct;         // grad_fts is asked for and rebuilt per table row
    float *gathered;     // grad_fts is asked for and staged here, at the head of the workspace; else null
    float *wd_partial;   // behind the staging region; null without a workspace
};
XdwGradPlan xdw_grad_plan(int b, int n_src, int rows_per_cloud, int k, int c1, int m, const float *grad_fts, void *workspace);
// the table's gradient by the plan's route, behind the entry's own launches
int xdw_grad_table(const XdwGradPlan &plan, int b, int n_src, int rows_per_cloud, int k, int c0, int c1, int m, const float *x,
                   const float *wd, const float *grad_out, const int *offsets, const int *entries, float *grad_fts, hf_stream_t stream);
// an empty batch (rows = 0): the weight and table gradients that are asked for are zero
int xdw_grad_empty(int b, int n_src, int k, int c0, int c1, int m, float *grad_fts, float *grad_wd, hipStream_t st);

}  // namespace hf
