// What the listwise launches share (head_listwise.hip; head_mined.hip: the same forward, the objective on a mined list): the arguments,
// the workgroup reductions in their fixed order, the forward that keeps the own domain's logits in LDS, and the objective on them.
#pragma once
#include "head_parts.h"

namespace amid {

#pragma clang fp contract(off)

struct ListwiseArgs {
    HeadArgs h;                // dp1 / dp2 of it: dz1 / dz2 [B, NI], written by the objective stage, read by the backward
    int kind;                  // 1 softmax, 2 BPR
    float* du;                 // [2, B, D]
};

constexpr int LW_MAX_NI = 1024;

// the eight waves' partials (one per wave in red[0 .. 8)) in the fixed order; every thread returns the same value.  Two barriers.
__device__ __forceinline__ float lw_block_sum(float v, float* __restrict__ red) {
    v = group_sum<64>(v);
    __syncthreads();                                   // (red may still be read from the previous reduction)
    if (lane_id() == 0) red[wave_id()] = v;
    __syncthreads();
    return ((red[0] + red[1]) + (red[2] + red[3])) + ((red[4] + red[5]) + (red[6] + red[7]));
}
__device__ __forceinline__ float lw_block_max(float v, float* __restrict__ red) {
    v = group_max<64>(v);
    __syncthreads();
    if (lane_id() == 0) red[wave_id()] = v;
    __syncthreads();
    return fmaxf(fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3])), fmaxf(fmaxf(red[4], red[5]), fmaxf(red[6], red[7])));
}

// scorer_fwd_part without the BCE: p1 / p2 by the very expressions of it (the same bits as amid_scorer_fwd_f32), and the own domain's
// logits kept in zs [NI]
__device__ __forceinline__ void listwise_fwd_part(const HeadArgs& a, const HeadLds& s, int b, int own, float* __restrict__ zs, const Tg tg) {
    const int hid = a.hid, NI = a.NI;
    user_half(a, s, tg);
    const int CH = s.chunk;
    for (int n0 = 0; n0 < NI; n0 += CH) {
        const int nn = min(CH, NI - n0);
        head_sync(s);
        item_half(a, s, b, n0, nn, tg);
        head_sync(s);
        for (int nd0 = 0; nd0 < nn * 2; nd0 += tg.n >> 5) {
            const int nd = nd0 + (tg.tid >> 5), j0 = tg.tid & 31;
            const bool on = nd < nn * 2;
            const int n = on ? nd >> 1 : 0, d = nd & 1;
            float zp = 0.f;
            if (on) for (int j = j0; j < hid; j += 32) zp = fmaf(a.w2[j], fmaxf(s.au[d * hid + j] + s.ci[n * (hid + 1) + j], 0.f), zp);
            const float z = group_sum<32>(zp) + a.b2[0];
            if (!on || j0 != 0) continue;
            const float p = 1.0f / (1.0f + expf(-z));
            (d ? a.p2 : a.p1)[(long long)b * NI + n0 + n] = p;
            if (d == own) zs[n0 + n] = z;
        }
    }
    __syncthreads();
}

// the row's objective on zs [NI]: loss_part[b], and dz / B into the own domain's dz row (zeros into the other's)
__device__ __forceinline__ void listwise_objective(const HeadArgs& a, int kind, int b, int own, const float* __restrict__ zs, float* __restrict__ red) {
    const int NI = a.NI, t = threadIdx.x;
    const float fB = (float)a.B;
    float* dz_own = (own ? a.dp2 : a.dp1) + (long long)b * NI;
    float* dz_oth = (own ? a.dp1 : a.dp2) + (long long)b * NI;
    for (int n = t; n < NI; n += 512) dz_oth[n] = 0.f;
    const float z0 = zs[0];
    if (kind == 1) {
        float m = -INFINITY;
        for (int n = t; n < NI; n += 512) m = fmaxf(m, zs[n]);
        m = lw_block_max(m, red);
        float e = 0.f;
        for (int n = t; n < NI; n += 512) e += expf(zs[n] - m);
        const float lse = m + logf(lw_block_sum(e, red));
        for (int n = t; n < NI; n += 512) dz_own[n] = (expf(zs[n] - lse) - (n == 0 ? 1.f : 0.f)) / fB;
        if (t == 0) a.loss_part[b] = (lse - z0) / fB;
    } else {
        const float fK = (float)(NI - 1);
        float l = 0.f, g = 0.f;
        for (int n = t; n < NI; n += 512) {
            if (n == 0) continue;
            const float x = zs[n] - z0;
            l += fmaxf(x, 0.f) + log1pf(expf(-fabsf(x)));
            const float gn = (1.0f / (1.0f + expf(-x))) / fK;
            g += gn;
            dz_own[n] = gn / fB;
        }
        l = lw_block_sum(l, red);
        g = lw_block_sum(g, red);
        if (t == 0) { dz_own[0] = -g / fB; a.loss_part[b] = (l / fK) / fB; }
    }
}

#pragma clang fp contract(fast)

}  // namespace amid
