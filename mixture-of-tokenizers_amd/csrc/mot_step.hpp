// mot_step.hpp -- what the decode-step kernels of the character mixer share (mot_swa_step.hip: attention + residuals,
// mot_ffn_step.hip: the feed-forward): the shape limits, the 16-byte lane load, the rounding of a value of a tensor of type T
// and the skinny product of R <= 16 staged rows with a weight matrix that is read once.
#pragma once
#include "mot_mix.hpp"

namespace mot {
namespace {

constexpr int kStepMaxRows = 16;
constexpr int kStepThreads = 256, kStepWaves = kStepThreads / 64;   // the two product kernels (512 threads, same session: 110 -> 93 us at B 16 in fp32, 24 -> 27 us replayed at B 1 in bf16)
constexpr int kStepCls = 4;                     // rows of the weight matrix a wave holds in flight
constexpr size_t kStepMaxLds = 128u << 10;      // the staged rows: R * dim (R * hdim) elements

template <typename T> struct StepVec;           // one 16-byte lane load of a weight row / of the staged rows
template <> struct StepVec<float> {
    static constexpr int N = 4;
    float4v q;
    __device__ __forceinline__ float get(int e) const { return q[e]; }
};
template <> struct StepVec<__bf16> {
    static constexpr int N = 8;
    bf16x8v q;
    __device__ __forceinline__ float get(int e) const { return (float)q[e]; }
};

template <typename T> __device__ __forceinline__ float step_round(float v) { return v; }          // a value of a tensor of type T
template <> __device__ __forceinline__ float step_round<__bf16>(float v) { return (float)(__bf16)v; }

// S[r][c] for r < n_rows, c in [c0, c0 + 4): sum_k xs[r][k] W[c][k], fp32 fused multiply-adds over the lane's slices in k order,
// then the wave's DPP sum; f(r, c, value) is called by lane c - c0 < 4.
template <typename T, int R, class F>
__device__ __forceinline__ void step_products(const T *__restrict__ xs, const T *__restrict__ W, int K, int c0, int n_rows, F &&f) {
    typedef StepVec<T> Vec;
    const int lane = threadIdx.x & 63, kvec = K / Vec::N;
    float acc[kStepCls][R];
#pragma unroll
    for (int c = 0; c < kStepCls; ++c)
#pragma unroll
        for (int r = 0; r < R; ++r) acc[c][r] = 0.f;
#pragma unroll 2
    for (int kv = lane; kv < kvec; kv += 64) {
        Vec w[kStepCls];
#pragma unroll
        for (int c = 0; c < kStepCls; ++c) w[c] = ((const Vec *)(W + (int64_t)(c0 + c) * K))[kv];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const Vec xv = ((const Vec *)(xs + r * K))[kv];
#pragma unroll
            for (int e = 0; e < Vec::N; ++e) {
                const float xe = xv.get(e);
#pragma unroll
                for (int c = 0; c < kStepCls; ++c) acc[c][r] = __builtin_fmaf(w[c].get(e), xe, acc[c][r]);
            }
        }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
        float s[kStepCls];
#pragma unroll
        for (int c = 0; c < kStepCls; ++c) s[c] = wave_sum(acc[c][r]);
        if (lane < kStepCls && r < n_rows) f(r, c0 + lane, lane == 0 ? s[0] : lane == 1 ? s[1] : lane == 2 ? s[2] : s[3]);
    }
}

}  // namespace
}  // namespace mot
