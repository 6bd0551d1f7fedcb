// mot_headrows.hpp -- what the V-wide row passes share (tokhead_rows of mot_tokhead.hip, plainhead_rows of mot_plainhead.hip): the
// limits and the geometry of a row pass, 16 bytes of a row of logits, the workgroup's fixed-order sums and the evaluation's share
// of a vector.  Device inline only; the launchers stay with their kernels.
#pragma once
#include "mot_headcore.hpp"

namespace mot {

constexpr int kMinV = 128, kMaxV = 262144, kMaxD = 2048;
constexpr int64_t kChunkBytes = 512ll << 20;      // the library's chunk: logits and u of a chunk stay below this
constexpr int kRowThreads = 1024;                 // workgroup of the row pass at wide rows; kRowThreadsSmall when a row has <= 1024 vectors
constexpr int kRowThreadsSmall = 256;
constexpr int kRowWavesMax = kRowThreads / 64;
constexpr int kRegV = 65536;                      // widest row the row pass keeps in registers between its two uses

// 16 bytes of a row of logits: 4 fp32 or 8 bf16
template <typename T>
struct LogitVec;
template <>
struct LogitVec<float> {
    static constexpr int N = 4;
    float4 q;
    __device__ __forceinline__ float get(int e) const { return e == 0 ? q.x : e == 1 ? q.y : e == 2 ? q.z : q.w; }
    __device__ __forceinline__ void put(const float *v) { q = make_float4(v[0], v[1], v[2], v[3]); }
};
template <>
struct LogitVec<__bf16> {
    static constexpr int N = 8;
    uint4 q;
    __device__ __forceinline__ float get(int e) const {
        const uint32_t w = e < 2 ? q.x : e < 4 ? q.y : e < 6 ? q.z : q.w;
        return __uint_as_float((e & 1) ? (w & 0xffff0000u) : (w << 16));
    }
    static __device__ __forceinline__ uint32_t pack(float lo, float hi) {   // two roundings to nearest even
        const __bf16 a = (__bf16)lo, b = (__bf16)hi;
        return (uint32_t)__builtin_bit_cast(unsigned short, a) | ((uint32_t)__builtin_bit_cast(unsigned short, b) << 16);
    }
    __device__ __forceinline__ void put(const float *v) { q = make_uint4(pack(v[0], v[1]), pack(v[2], v[3]), pack(v[4], v[5]), pack(v[6], v[7])); }
};

// workgroup size and vectors per thread of a row pass over V classes of T: 256 threads while a row has at most 1024 vectors
template <typename T>
inline void rows_geometry(int V, int &threads, int &vecs_per_thread) {
    const int nvec = V / LogitVec<T>::N;
    threads = nvec <= 4 * kRowThreadsSmall ? kRowThreadsSmall : kRowThreads;
    vecs_per_thread = (nvec + threads - 1) / threads;
}

// sum over the workgroup in a fixed order: the waves' DPP sums, then the waves in index order.  `sh` holds one float per wave and is
// used by one sum only, so a single barrier suffices.
__device__ __forceinline__ float rows_block_sum(float v, float *sh) {
    const int nw = blockDim.x >> 6;
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    float s = 0.f;
    for (int w = 0; w < nw; ++w) s += sh[w];
    return s;
}

// the workgroup's largest value, laid out as rows_block_sum: the waves' DPP maxima, then the waves in index order
__device__ __forceinline__ float rows_block_max(float v, float *sh) {
    const int nw = blockDim.x >> 6;
    v = wave_max(v);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    float m = sh[0];
    for (int w = 1; w < nw; ++w) m = fmaxf(m, sh[w]);
    return m;
}

// the evaluation's share of one vector whose first class is cls0, on the logits as stored: the largest so far with its class (a
// thread meets its classes in ascending order, so `>` keeps the lowest class of equal logits) and the count of those above sy
template <typename T>
__device__ __forceinline__ void vec_top(const LogitVec<T> &a, int cls0, float sy, float &best, int &best_cls, int &above) {
#pragma unroll
    for (int e = 0; e < LogitVec<T>::N; ++e) {
        const float s = a.get(e);
        if (s > best) {
            best = s;
            best_cls = cls0 + e;
        }
        above += s > sy ? 1 : 0;
    }
}

}  // namespace mot
