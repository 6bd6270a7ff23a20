// The item-item similarity of neighbors.hip and diversify.hip, stated once: a score is a function of its two rows and the metric only, and
// both files give the same bits for the same two rows.
//   dot(a, b)     the accumulator starts at 0 and takes the products of elements s, D/4 + s, 2 D/4 + s, 3 D/4 + s for s = 0 .. D/4 - 1, one
//                 fmaf each, in that order.  neighbors.hip runs it as D / 4 v_mfma_f32_16x16x4_f32 (sim_mfma: an MFMA is bitwise the fmaf
//                 chain over its k-slots 0 .. 3, and k-slot g walks quarter g of the row); diversify.hip as the plain chain (sim_dot_chain)
//   inverse norm  1 / max(|row|, 1e-8): eight lanes a row, each an fmaf chain over its D / 8 elements, joined by group_sum<8> (sim_inv_norm)
//   cosine        (dot * inv(query)) * inv(candidate), in that order (sim_cosine)
#pragma once
#include "common.h"

namespace amid {

#pragma clang fp contract(off)

__device__ __forceinline__ f32x4 sim_mfma(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

// Every lane of a group of eight consecutive lanes calls this with the same row (null: no such row, 0) and its part 0 .. 7.
template <int D>
__device__ __forceinline__ float sim_inv_norm(const float* row, int part) {
    float ss = 0.f;
    if (row != nullptr) {
#pragma unroll
        for (int i = 0; i < D / 32; ++i) {
            const float4 v = ld4(row + part * (D / 8) + 4 * i);
            ss = fmaf(v.x, v.x, ss); ss = fmaf(v.y, v.y, ss); ss = fmaf(v.z, v.z, ss); ss = fmaf(v.w, v.w, ss);
        }
    }
    ss = group_sum<8>(ss);
    return row != nullptr ? 1.0f / fmaxf(sqrtf(ss), 1e-8f) : 0.f;
}

__device__ __forceinline__ float sim_cosine(float dot, float inv_query, float inv_cand) { return (dot * inv_query) * inv_cand; }

// The chain of one thread: x[g][i] = float4 i of quarter g of its own row (registers), b = the other row (16-byte aligned, LDS or global).
template <int D>
__device__ __forceinline__ float sim_dot_chain(const float4 (&x)[4][D / 16], const float* b) {
    constexpr int DQ = D / 4;
    float acc = 0.f;
#pragma unroll
    for (int i = 0; i < DQ / 4; ++i) {
        const float4 b0 = ld4(b + 4 * i), b1 = ld4(b + DQ + 4 * i), b2 = ld4(b + 2 * DQ + 4 * i), b3 = ld4(b + 3 * DQ + 4 * i);
        acc = fmaf(x[0][i].x, b0.x, acc); acc = fmaf(x[1][i].x, b1.x, acc); acc = fmaf(x[2][i].x, b2.x, acc); acc = fmaf(x[3][i].x, b3.x, acc);
        acc = fmaf(x[0][i].y, b0.y, acc); acc = fmaf(x[1][i].y, b1.y, acc); acc = fmaf(x[2][i].y, b2.y, acc); acc = fmaf(x[3][i].y, b3.y, acc);
        acc = fmaf(x[0][i].z, b0.z, acc); acc = fmaf(x[1][i].z, b1.z, acc); acc = fmaf(x[2][i].z, b2.z, acc); acc = fmaf(x[3][i].z, b3.z, acc);
        acc = fmaf(x[0][i].w, b0.w, acc); acc = fmaf(x[1][i].w, b1.w, acc); acc = fmaf(x[2][i].w, b2.w, acc); acc = fmaf(x[3][i].w, b3.w, acc);
    }
    return acc;
}

#pragma clang fp contract(fast)

}  // namespace amid
