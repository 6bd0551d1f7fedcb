// mot_group.hip -- counting sort of positions by a small integer key, and the zeroing kernel it starts with.
// launch_group_positions orders the token positions by token id for the scatter kernels of mot_backward.hip; mot_token_order
// (mot_capi.hip) and the cross-attention backward (mot_attn.hip) call it as well.
// launch_zero_words clears its counters, and workspace of the MEAN backward (mot_bwd_mean.hip), cross-attention (mot_attn.hip),
// the byte head (mot_head.hip) and byte self-attention (mot_bsa.hip): a kernel, since a memset node aborts on graph replay
// with this runtime.
#include "mot_mix.hpp"

namespace mot {

// ---- grouping of the token positions by (clamped) token id: a counting sort in three small kernels.
// bwd_rank_kernel: a workgroup sorts (token << 11 | index) for 2048 positions in LDS (bitonic), so equal tokens become
// runs; the head of a run reserves the run's places in the token's group with ONE atomicAdd(counts[token], length)
// (a hot token costs one atomic per workgroup, not one per occurrence) and every position gets its rank in the group.
// bwd_scan_kernel: group starts.  bwd_place_kernel: pos_sorted[start[token] + rank] = position (no atomics).
constexpr int kRankThreads = 512;
__device__ __forceinline__ int lower_bound_u32(const uint32_t *a, int n, uint32_t v) {   // first index with a[i] >= v
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (a[mid] < v) lo = mid + 1; else hi = mid;
    }
    return lo;
}
__global__ __launch_bounds__(kThreads) void zero_i32_kernel(int32_t *__restrict__ p, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kThreads) p[i] = 0;
}

int launch_zero_words(void *p, int64_t n_words, hipStream_t stream) {
    if (n_words <= 0) return MOT_OK;
    int64_t blocks = (n_words + kThreads - 1) / kThreads;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(zero_i32_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, stream, (int32_t *)p, n_words);
    return check_launch("zero_i32_kernel");
}

template <int kRankChunk>   // positions per workgroup: 2048, or 512 when there are too few positions to fill the chip with 2048s
__global__ __launch_bounds__(kRankThreads) void bwd_rank_kernel(const int32_t *__restrict__ tokens, int64_t n, int64_t rows,
                                                                int32_t *__restrict__ counts, int32_t *__restrict__ rank,
                                                                uint32_t *status) {
    __shared__ uint32_t skey[kRankChunk];
    __shared__ int32_t runbase[kRankChunk];
    const int tid = threadIdx.x;
    const int64_t base = (int64_t)blockIdx.x * kRankChunk;
    for (int i = tid; i < kRankChunk; i += kRankThreads) {
        uint32_t key = 0xffffffffu;
        if (base + i < n) {
            uint32_t t = (uint32_t)tokens[base + i];
            if ((uint64_t)t >= (uint64_t)rows) { if (status) atomicOr(status, kStatusTokenOor); t = 0; }
            key = (t << 11) | (uint32_t)i;
        }
        skey[i] = key;
    }
    __syncthreads();
    for (int k = 2; k <= kRankChunk; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int p = tid; p < kRankChunk / 2; p += kRankThreads) {
                const int i = ((p & ~(j - 1)) << 1) | (p & (j - 1)), ixj = i | j;
                const uint32_t x = skey[i], y = skey[ixj];
                if ((x > y) == ((i & k) == 0)) { skey[i] = y; skey[ixj] = x; }
            }
            __syncthreads();
        }
    constexpr int kPer = kRankChunk / kRankThreads;
    int head[kPer];
#pragma unroll
    for (int r = 0; r < kPer; ++r) {
        const int si = tid + r * kRankThreads;
        const uint32_t key = skey[si];
        head[r] = -1;
        if (key == 0xffffffffu) continue;
        const uint32_t tok = key >> 11;
        const int h = (si == 0 || (skey[si - 1] >> 11) != tok) ? si : lower_bound_u32(skey, si, tok << 11);
        head[r] = h;
        if (h == si) {
            const int e = lower_bound_u32(skey, kRankChunk, (tok + 1) << 11);   // padding keys are larger than any token's
            runbase[si] = atomicAdd(&counts[tok], e - si);
        }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < kPer; ++r) {
        const int si = tid + r * kRankThreads;
        if (head[r] < 0) continue;
        rank[base + (skey[si] & 2047)] = runbase[head[r]] + (si - head[r]);
    }
}

__global__ __launch_bounds__(kThreads) void bwd_place_kernel(const int32_t *__restrict__ tokens, int64_t n, int64_t rows,
                                                             const int32_t *__restrict__ starts, const int32_t *__restrict__ rank,
                                                             int32_t *__restrict__ pos_sorted, int32_t *__restrict__ tok_sorted) {
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kThreads) {
        int t = tokens[i];
        if ((uint64_t)(uint32_t)t >= (uint64_t)rows) t = 0;
        const int32_t at = starts[t] + rank[i];
        pos_sorted[at] = (int32_t)i;
        tok_sorted[at] = t;
    }
}

// exclusive scan of counts[0..rows) into starts.  Workgroup b owns the 1024 counts of tile b: it first sums everything in
// front of its tile (coalesced reads of an L2-resident array, at most a few hundred KB), then scans its own tile.
__global__ __launch_bounds__(1024) void bwd_scan_kernel(const int32_t *__restrict__ counts, int64_t rows,
                                                        int32_t *__restrict__ starts) {
    __shared__ int32_t wsum[16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t t0 = (int64_t)blockIdx.x * 1024;
    int32_t before = 0;
    for (int64_t i = tid; i < t0; i += 1024) before += counts[i];
    const int64_t i = t0 + tid;
    const int32_t own = i < rows ? counts[i] : 0;
    const int32_t incl = wave_incl_add(own, lane);
    const int32_t bsum = wave_incl_add(before, lane);
    if (lane == 63) wsum[wave] = incl + bsum;     // this wave's share of (everything before the tile + the tile)
    __syncthreads();
    int32_t off = incl - own;
    for (int w = 0; w < 16; ++w) off += w < wave ? wsum[w] : 0;
    // the `before` parts of the later waves belong in front of every element of the tile as well
    __shared__ int32_t bpart[16];
    if (lane == 63) bpart[wave] = bsum;
    __syncthreads();
    for (int w = wave; w < 16; ++w) off += bpart[w];
    if (i < rows) starts[i] = off;
}

// The counting sort by itself: positions 0..n-1 grouped by ids[position] (clamped into [0, rows)); `ws_ints` holds
// group_positions_ws_ints(n, rows) int32.  *pos_sorted / *id_sorted point into it.
size_t group_positions_ws_ints(int64_t n, int64_t rows) { return 2 * (size_t)rows + 3 * (size_t)n; }
int launch_group_positions(const int32_t *ids, int64_t n, int64_t rows, int32_t *ws_ints, const int32_t **pos_sorted_out, const int32_t **id_sorted_out,
                           uint32_t *status, hipStream_t stream) {
    if (rows >= (1 << 21) - 1) return set_error(MOT_EUNSUPPORTED, "group_positions: %lld rows (>= 2^21 - 1) are not built", (long long)rows);
    int32_t *counts = ws_ints, *starts = counts + rows, *rank = starts + rows, *pos_sorted = rank + n, *id_sorted = pos_sorted + n;
    int rc;
    if ((rc = launch_zero_words(counts, rows, stream))) return rc;
    const int rank_chunk = n >= 256 * 2048 ? 2048 : 512;
    const int64_t rb = (n + rank_chunk - 1) / rank_chunk;
    int64_t pb = (n + kThreads - 1) / kThreads;
    if (pb > 2048) pb = 2048;
    if (rb > 0x7fffffffLL) return set_error(MOT_EUNSUPPORTED, "group_positions: too many positions");
    if (n > 0) {
        if (rank_chunk == 2048)
            hipLaunchKernelGGL(bwd_rank_kernel<2048>, dim3((unsigned)rb), dim3(kRankThreads), 0, stream, ids, n, rows, counts, rank, status);
        else
            hipLaunchKernelGGL(bwd_rank_kernel<512>, dim3((unsigned)rb), dim3(kRankThreads), 0, stream, ids, n, rows, counts, rank, status);
        hipLaunchKernelGGL(bwd_scan_kernel, dim3((unsigned)((rows + 1023) / 1024)), dim3(1024), 0, stream, counts, rows, starts);
        hipLaunchKernelGGL(bwd_place_kernel, dim3((unsigned)pb), dim3(kThreads), 0, stream, ids, n, rows, starts, rank, pos_sorted, id_sorted);
        if ((rc = check_launch("group_positions kernels"))) return rc;
    }
    *pos_sorted_out = pos_sorted;
    *id_sorted_out = id_sorted;
    return MOT_OK;
}

}  // namespace mot
