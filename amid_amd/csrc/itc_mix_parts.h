// The arithmetic of InterComp's mix in its 512-thread form (csrc/intercomp.hip itc_mix_fwd_fast_kernel: B <= 256, D 64 / 128 -- 16 row groups
// of 32 lanes, 8 waves), as single-thread pieces for the two places that must agree bit for bit: that kernel, and the evaluation head's prologue
// (csrc/eval_head.hip), where every workgroup recomputes the batch-wide values for its own sample's domain.
#pragma once
#include "common.h"

namespace amid {

// Every expression compiles to the operations as written (fmaf where an fma is meant -- the ones the mix kernel's build contracted before this
// header existed): what the compiler contracts on its own depends on the code around it.  (Restored at the end of this header.)
#pragma clang fp contract(off)

constexpr int MIXF_RG = 16, MIXF_K = 16;          // rows per row group: B <= MIXF_RG * MIXF_K; W_nn rows per row group: 2 D / 16 <= 16

__device__ __forceinline__ float block_reduce_sum(float v, float* red) {      // 1024 threads max; all threads get the result
    v = group_sum<64>(v);
    __syncthreads();
    if (lane_id() == 0) red[wave_id()] = v;
    __syncthreads();
    float s = 0.f;
    for (int k = 0; k < (int)(blockDim.x >> 6); ++k) s += red[k];
    return s;
}
__device__ __forceinline__ float block_reduce_max(float v, float* red) {
    v = group_max<64>(v);
    __syncthreads();
    if (lane_id() == 0) red[wave_id()] = v;
    __syncthreads();
    float s = -INFINITY;
    for (int k = 0; k < (int)(blockDim.x >> 6); ++k) s = fmaxf(s, red[k]);
    return s;
}

// row j's term of the batch softmax's denominator, and its gate (model_seq.py:490-491): m = max_j s_j, l = sum_j exp(s_j - m) -- a thread's own
// terms, then group_sum<64>, then the waves in order
__device__ __forceinline__ float itc_softmax_term(float s_j, float m) { return expf(s_j - m); }
__device__ __forceinline__ float itc_gate(float s_j, float m, float l, float threshold) { return (expf(s_j - m) / l > threshold) ? 1.f : 0.f; }

// z_g += (w_bs_g[j] gate_j) u_raw[other(g)][j]: one row of a row group's chain (rows rg, rg + 16, ... in order; then the 16 partials in order)
__device__ __forceinline__ void itc_z_step(float4& acc, float w, const float4& v) {
    acc.x = fmaf(w, v.x, acc.x); acc.y = fmaf(w, v.y, acc.y); acc.z = fmaf(w, v.z, acc.z); acc.w = fmaf(w, v.w, acc.w);
}

// c_g[o] = W_nn_g[o, :] . z_g + b_nn_g[o] sum_j w_g[j] + b_bs_g: a lane's quad of the row, the 32 lanes joined by a tree over the lane bits
// 16, 8, 4, 2, 1 (itc_c_tree; the kernel's butterfly over 16 rows is that tree for every row), then the bias terms
__device__ __forceinline__ float itc_c_dot4(const float4& w, const float4& z) { return fmaf(w.x, z.x, fmaf(w.y, z.y, fmaf(w.z, z.z, w.w * z.w))); }
__device__ __forceinline__ float itc_c_tree(float v) {
#pragma unroll
    for (int bit = 16; bit >= 1; bit >>= 1) v = v + __shfl_xor(v, bit, 64);
    return v;
}
__device__ __forceinline__ float itc_c_finish(float dot, float b_nn, float sw, float b_bs) { return fmaf(b_nn, sw, dot) + b_bs; }

// u = 0.5 u_raw + 0.5 c: the mean over the 2T rows of cat(f, group)  (:432-434, :495)
__device__ __forceinline__ float itc_mix(float own, float c) { return fmaf(c, 0.5f, own * 0.5f); }

#pragma clang fp contract(fast)

}  // namespace amid
