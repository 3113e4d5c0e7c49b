// xconv_common.h -- what the fused X-Conv kernels of xconv.hip and their BatchNorm-folding twins of xconv_bn.hip share: the device
// helpers of the channel-pair / lane-per-channel mappings (moved here from xconv.hip as they stood) and the launch geometry and
// table-gradient launcher that xconv.hip defines.
#pragma once
#include "hf_common.h"

#include <initializer_list>

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

}  // namespace hf
