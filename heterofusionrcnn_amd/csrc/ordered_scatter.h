// ordered_scatter.h -- the ordered scatter-add shared by glue.hip (hf_project_gather_grad_ordered) and roi_image.hip
// (hf_crop_and_resize_grad_ordered): kernel templates over an entry functor and one host launcher.
//
// One idea: `entries` terms of c floats in a fixed order, each with a target row key(e) in [0, targets) or none (-1);
//   out[t] = sum over { e : key(e) == t } of term(e), added in ASCENDING e, fp32, from +0.0f, one rounding per add,
// which is what a sequential loop over e gives on a zero-filled map, and what fp32 atomics give only up to the order.  Every
// row of `out` is written exactly once (a row that nothing names becomes +0): no zero fill of the map, no read-modify-write.
//
// The functor F:  __device__ int key(int e) const           target row of entry e, -1 for an entry that adds nothing
//                 template <int VEC> __device__ void terms(int e, int ch, float *v) const
//                                                            channels [ch, ch + VEC) of its term, in the arithmetic the atomic kernel
//                                                            uses; VEC = 4 only where vec4 was passed to the launcher
//
// Launches, all on the caller's stream, one chain (capturable; no workgroup waits on another):
//   os_zero_kernel          the per-target counters and the long-list counter := 0 (a kernel, not a memset node: roi_image.hip)
//   os_keys_kernel          keys[e] = key(e); cursor[key] += 1 by INTEGER atomics (a count does not depend on their order)
//   os_scan_chunks_kernel   exclusive scan of the counts inside chunks of kOsChunk targets, in place; the chunk totals; targets
//                           with more than kOsThreadSort entries claim a slot of the long-list worklist (its order is free:
//                           every list is ordered on its own)
//   os_scan_bases_kernel    exclusive scan of the chunk totals by one workgroup: list t starts at chunk_base[t / kOsChunk] + cursor[t]
//   os_fill_kernel          entry e claims slot cursor[key]++ of its list.  Afterwards cursor[t] is the END of list t inside its
//                           chunk, which is the start of list t + 1: os_list reads both from the one map.
//   os_order_short_kernel   one thread per target: lists of 2 .. kOsThreadSort ids sorted ascending in place (insertion sort,
//                           at most kOsThreadSort (kOsThreadSort - 1) / 2 moves)
//   os_order_long_kernel    one 1024-thread workgroup per long list (grid-stride over the worklist): a bitonic network whose
//                           comparators all put the smaller id at the lower index, so a list of any length sorts as if padded
//                           with +inf to a power of two (a comparator that reaches past the end is a no-op).  Up to kOsLdsSort
//                           ids in LDS, longer lists in place in the workspace.  O(n log^2 n / 1024) per list: 16 384 entries
//                           on one pixel are 105 stages of 8 comparators a thread.
//   os_reduce_kernel        a team of tl lanes per target, VEC floats a lane (4 where c % 4 == 0 and both the terms and the map are
//                           16-byte aligned, else 1), tl = min(64, c / VEC rounded up to a power of two), walks the sorted ids, adds
//                           the terms (rows of c contiguous floats) four loads at a time and writes the row once.
// The slot an entry claims depends on the order of the atomics; the sorted list, and so the sum, does not.
//
// Workspace (os_layout, bytes, every part 16-byte aligned): long-list counter | cursor[targets] | chunk_base[chunks] |
// keys[entries] | slots[entries] | worklist[entries / (kOsThreadSort + 1) + 1].  targets and entries fit int.
#pragma once
#include <limits.h>

#include "hf_common.h"

namespace hf {

constexpr int kOsScanThreads = 1024;                 // block_exclusive_scan's workgroup
constexpr int kOsChunk = kOsScanThreads * 4;         // targets per workgroup of os_scan_chunks_kernel
constexpr int kOsThreadSort = 16;                    // longest list that the thread of its target sorts alone
constexpr int kOsLdsSort = 4096;                     // longest list that os_order_long_kernel sorts in LDS
constexpr int kOsSortThreads = 1024;

struct OsLayout {
    size_t counter, cursor, chunk_base, keys, slots, worklist, total;   // byte offsets, and the size of it all
};

inline size_t os_round16(size_t bytes) { return (bytes + 15) / 16 * 16; }

inline OsLayout os_layout(int targets, int entries)
{
    OsLayout l;
    const size_t chunks = (static_cast<size_t>(targets) + kOsChunk - 1) / kOsChunk;
    l.counter = 0;
    l.cursor = 16;
    l.chunk_base = l.cursor + os_round16(sizeof(int) * static_cast<size_t>(targets));
    l.keys = l.chunk_base + os_round16(sizeof(int) * chunks);
    l.slots = l.keys + os_round16(sizeof(int) * static_cast<size_t>(entries));
    l.worklist = l.slots + os_round16(sizeof(int) * static_cast<size_t>(entries));
    l.total = l.worklist + os_round16(sizeof(int) * (static_cast<size_t>(entries) / (kOsThreadSort + 1) + 1));
    return l;
}

// the counts live in whole 16-byte pieces (os_layout rounds the map up), so the last piece may cover the padding
static __global__ __launch_bounds__(256) void os_zero_kernel(int nvec, int *__restrict__ cursor, int *__restrict__ counter)
{
    typedef int ivec4 __attribute__((ext_vector_type(4)));
    ivec4 *v = reinterpret_cast<ivec4 *>(cursor);
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < nvec; i += gridDim.x * blockDim.x) v[i] = ivec4{ 0, 0, 0, 0 };
    if (blockIdx.x == 0 && threadIdx.x == 0) *counter = 0;
}

template <class F>
__global__ __launch_bounds__(256) void os_keys_kernel(F f, int entries, int *__restrict__ keys, int *__restrict__ cursor)
{
    for (long long e = blockIdx.x * blockDim.x + threadIdx.x; e < entries; e += gridDim.x * blockDim.x) {
        const int k = f.key(static_cast<int>(e));
        keys[e] = k;
        if (k >= 0) atomicAdd(cursor + k, 1);
    }
}

static __global__ __launch_bounds__(kOsScanThreads) void os_scan_chunks_kernel(int targets, int *__restrict__ cursor,
                                                                        int *__restrict__ chunk_base, int *__restrict__ worklist,
                                                                        int *__restrict__ counter)
{
    __shared__ int wsum[16];
    const long long t0 = blockIdx.x * static_cast<long long>(kOsChunk) + threadIdx.x * 4;
    int n[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        n[i] = t0 + i < targets ? cursor[t0 + i] : 0;
        if (n[i] > kOsThreadSort) worklist[atomicAdd(counter, 1)] = static_cast<int>(t0 + i);
    }
    int total;
    int at = block_exclusive_scan(n[0] + n[1] + n[2] + n[3], wsum, &total);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (t0 + i < targets) cursor[t0 + i] = at;
        at += n[i];
    }
    if (threadIdx.x == 0) chunk_base[blockIdx.x] = total;
}

static __global__ __launch_bounds__(kOsScanThreads) void os_scan_bases_kernel(int chunks, int *__restrict__ chunk_base)
{
    __shared__ int wsum[16];
    int carry = 0;
    for (int i0 = 0; i0 < chunks; i0 += kOsScanThreads) {
        const int i = i0 + threadIdx.x;
        int total;
        const int at = block_exclusive_scan(i < chunks ? chunk_base[i] : 0, wsum, &total);
        if (i < chunks) chunk_base[i] = carry + at;
        carry += total;
    }
}

static __global__ __launch_bounds__(256) void os_fill_kernel(int entries, const int *__restrict__ keys, int *__restrict__ cursor,
                                                      const int *__restrict__ chunk_base, int *__restrict__ slots)
{
    for (long long e = blockIdx.x * blockDim.x + threadIdx.x; e < entries; e += gridDim.x * blockDim.x) {
        const int k = keys[e];
        if (k >= 0) slots[chunk_base[k / kOsChunk] + atomicAdd(cursor + k, 1)] = static_cast<int>(e);
    }
}

// list t after os_fill_kernel: its length, and where it starts in `slots`
__device__ __forceinline__ int os_list(int t, const int *__restrict__ cursor, const int *__restrict__ chunk_base, int *start)
{
    const int lo = t % kOsChunk ? cursor[t - 1] : 0;
    *start = chunk_base[t / kOsChunk] + lo;
    return cursor[t] - lo;
}

static __global__ __launch_bounds__(256) void os_order_short_kernel(int targets, const int *__restrict__ cursor,
                                                             const int *__restrict__ chunk_base, int *slots)
{
    for (long long t = blockIdx.x * blockDim.x + threadIdx.x; t < targets; t += gridDim.x * blockDim.x) {
        int start;
        const int n = os_list(static_cast<int>(t), cursor, chunk_base, &start);
        if (n < 2 || n > kOsThreadSort) continue;
        int *a = slots + start;
        for (int i = 1; i < n; ++i) {
            const int v = a[i];
            int j = i - 1;
            for (; j >= 0 && a[j] > v; --j) a[j + 1] = a[j];
            a[j + 1] = v;
        }
    }
}

__device__ __forceinline__ void os_compare(int *a, int lo, int hi, int n)
{
    if (hi >= n) return;        // the upper end is padding: +inf stays where it is
    const int x = a[lo], y = a[hi];
    if (x > y) { a[lo] = y; a[hi] = x; }
}

// ascending sort of a[0, n) by the whole workgroup; a in LDS or in global memory
__device__ __forceinline__ void os_bitonic_sort(int *a, int n)
{
    int m = 2;
    while (m < n) m <<= 1;
    for (int size = 2; size <= m; size <<= 1) {
        const int half = size >> 1;
        for (int q = threadIdx.x; q < (m >> 1); q += blockDim.x) {      // the two halves of a block, the upper one mirrored
            const int blk = q / half, off = q - blk * half;
            os_compare(a, blk * size + off, blk * size + size - 1 - off, n);
        }
        __syncthreads();
        for (int stride = half >> 1; stride > 0; stride >>= 1) {
            for (int q = threadIdx.x; q < (m >> 1); q += blockDim.x) {
                const int lo = 2 * stride * (q / stride) + q % stride;
                os_compare(a, lo, lo + stride, n);
            }
            __syncthreads();
        }
    }
}

static __global__ __launch_bounds__(kOsSortThreads) void os_order_long_kernel(int capacity, const int *__restrict__ cursor,
                                                                       const int *__restrict__ chunk_base, int *slots,
                                                                       const int *__restrict__ worklist,
                                                                       const int *__restrict__ counter)
{
    __shared__ int lds[kOsLdsSort];
    const int nlong = min(*counter, capacity);
    for (int i = blockIdx.x; i < nlong; i += gridDim.x) {
        int start;
        const int n = os_list(worklist[i], cursor, chunk_base, &start);
        int *a = slots + start;
        if (n <= kOsLdsSort) {
            for (int q = threadIdx.x; q < n; q += blockDim.x) lds[q] = a[q];
            __syncthreads();
            os_bitonic_sort(lds, n);
            for (int q = threadIdx.x; q < n; q += blockDim.x) a[q] = lds[q];
            __syncthreads();
        } else {
            os_bitonic_sort(a, n);
        }
    }
}

// VEC floats of a row per lane (4: 16-byte loads and stores; 1: any c and alignment), tl lanes per target
template <class F, int VEC>
__global__ __launch_bounds__(256) void os_reduce_kernel(F f, int targets, int c, int tl_shift, const int *__restrict__ cursor,
                                                        const int *__restrict__ chunk_base, const int *__restrict__ slots,
                                                        float *__restrict__ out)
{
    const int tl = 1 << tl_shift, cv = c / VEC;
    const int l = threadIdx.x & (tl - 1);
    const int teams = static_cast<int>((static_cast<long long>(gridDim.x) * blockDim.x) >> tl_shift);
    for (long long t = (blockIdx.x * static_cast<long long>(blockDim.x) + threadIdx.x) >> tl_shift; t < targets; t += teams) {
        int start;
        const int n = os_list(static_cast<int>(t), cursor, chunk_base, &start);
        const int *ids = slots + start;
        for (int lv = l; lv < cv; lv += tl) {
            const int ch = lv * VEC;
            float acc[VEC];
#pragma unroll
            for (int i = 0; i < VEC; ++i) acc[i] = 0.0f;
            int a = 0;
            for (; a + 4 <= n; a += 4) {      // four independent row loads, then the adds in list order
                float v[4][VEC];
#pragma unroll
                for (int k = 0; k < 4; ++k) f.template terms<VEC>(ids[a + k], ch, v[k]);
#pragma unroll
                for (int k = 0; k < 4; ++k)
#pragma unroll
                    for (int i = 0; i < VEC; ++i) acc[i] += v[k][i];
            }
            for (; a < n; ++a) {
                float v[VEC];
                f.template terms<VEC>(ids[a], ch, v);
#pragma unroll
                for (int i = 0; i < VEC; ++i) acc[i] += v[i];
            }
            float *dst = out + t * c + ch;
            if constexpr (VEC == 4) *reinterpret_cast<float4 *>(dst) = make_float4(acc[0], acc[1], acc[2], acc[3]);
            else dst[0] = acc[0];
        }
    }
}

// ---- host launcher: shapes and the workspace are checked by the entry points; targets > 0, entries >= 0, both fit int;
// vec4: c % 4 == 0 and the functor's rows and `out` are 16-byte aligned ----

template <class F>
inline int launch_ordered_scatter(const F &f, int targets, int entries, int c, bool vec4, float *out, void *workspace, hipStream_t st)
{
    const OsLayout lay = os_layout(targets, entries);
    char *ws = static_cast<char *>(workspace);
    int *counter = reinterpret_cast<int *>(ws + lay.counter), *cursor = reinterpret_cast<int *>(ws + lay.cursor);
    int *chunk_base = reinterpret_cast<int *>(ws + lay.chunk_base), *keys = reinterpret_cast<int *>(ws + lay.keys);
    int *slots = reinterpret_cast<int *>(ws + lay.slots), *worklist = reinterpret_cast<int *>(ws + lay.worklist);
    const int chunks = div_up(targets, kOsChunk);
    const int nvec = div_up(targets, 4);
    int rc;
    hipLaunchKernelGGL(os_zero_kernel, dim3(grid_for(nvec, 256)), dim3(256), 0, st, nvec, cursor, counter);
    if ((rc = launch_status()) != HF_OK) return rc;
    if (entries > 0) {
        hipLaunchKernelGGL((os_keys_kernel<F>), dim3(grid_for(entries, 256)), dim3(256), 0, st, f, entries, keys, cursor);
        if ((rc = launch_status()) != HF_OK) return rc;
    }
    hipLaunchKernelGGL(os_scan_chunks_kernel, dim3(chunks), dim3(kOsScanThreads), 0, st, targets, cursor, chunk_base, worklist,
                       counter);
    if ((rc = launch_status()) != HF_OK) return rc;
    hipLaunchKernelGGL(os_scan_bases_kernel, dim3(1), dim3(kOsScanThreads), 0, st, chunks, chunk_base);
    if ((rc = launch_status()) != HF_OK) return rc;
    if (entries > 0) {
        hipLaunchKernelGGL(os_fill_kernel, dim3(grid_for(entries, 256)), dim3(256), 0, st, entries, keys, cursor, chunk_base, slots);
        if ((rc = launch_status()) != HF_OK) return rc;
        hipLaunchKernelGGL(os_order_short_kernel, dim3(grid_for(targets, 256)), dim3(256), 0, st, targets, cursor, chunk_base, slots);
        if ((rc = launch_status()) != HF_OK) return rc;
        const int capacity = entries / (kOsThreadSort + 1) + 1;
        hipLaunchKernelGGL(os_order_long_kernel, dim3(capacity < kNumCU ? capacity : kNumCU), dim3(kOsSortThreads), 0, st, capacity,
                           cursor, chunk_base, slots, worklist, counter);
        if ((rc = launch_status()) != HF_OK) return rc;
    }
    const int cv = vec4 ? c / 4 : c;
    int tl_shift = 0;
    while ((1 << tl_shift) < cv && tl_shift < 6) ++tl_shift;
    long long grid = (static_cast<long long>(targets) + (256 >> tl_shift) - 1) / (256 >> tl_shift);
    if (grid > kNumCU * 64ll) grid = kNumCU * 64ll;
    if (vec4)
        hipLaunchKernelGGL((os_reduce_kernel<F, 4>), dim3(static_cast<unsigned>(grid)), dim3(256), 0, st, f, targets, c, tl_shift, cursor,
                           chunk_base, slots, out);
    else
        hipLaunchKernelGGL((os_reduce_kernel<F, 1>), dim3(static_cast<unsigned>(grid)), dim3(256), 0, st, f, targets, c, tl_shift, cursor,
                           chunk_base, slots, out);
    return launch_status();
}

}  // namespace hf
