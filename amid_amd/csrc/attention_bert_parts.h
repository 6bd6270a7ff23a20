// The forward attention core of the BERT4Rec shape (bidirectional, key mask, 4 heads of 32, T <= 64) per (query tile, head), shared by
// attention_mfma_bert.hip (operands from global memory, a launch of its own) and bert_seq_infer.hip (K / V images in LDS, q in registers,
// inside the one-launch encoder).  The result of a (query tile, head) pair depends on that tile's q, the sequence's k and v and the mask
// bits only, and both callers run THIS code on them: the same bits.
#pragma once
#include "attention_mfma.h"

namespace amid {

constexpr int BHD = 32;

__device__ __forceinline__ f32x4 frag2(const float4 (&a)[2], const float4 (&b)[2], f32x4 c) {
    c = mfma_frag(a[0], b[0], c);
    return mfma_frag(a[1], b[1], c);
}

// bit (kj * 4 + r) of the result: key n = kj * 16 + 4 gq + r is inside the sequence (valid) / also visible (ok)
__device__ __forceinline__ void key_bits(const unsigned char* __restrict__ kk, int T, int gq, unsigned& valid, unsigned& ok) {
    // (the sixteen mask bytes of the lane are requested back to back, clamped instead of branched around: behind a branch per key each
    // byte load waited out its own round trip -- sixteen dependent L2 latencies at the head of every wave)
    unsigned char kb[16];
#pragma unroll
    for (int kj = 0; kj < 4; ++kj)
#pragma unroll
        for (int r = 0; r < 4; ++r) kb[kj * 4 + r] = kk != nullptr ? kk[min(kj * 16 + 4 * gq + r, T - 1)] : (unsigned char)1;
    valid = 0; ok = 0;
#pragma unroll
    for (int kj = 0; kj < 4; ++kj)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int n = kj * 16 + 4 * gq + r;
            const unsigned bit = n < T ? 1u << (kj * 4 + r) : 0u;
            valid |= bit;
            ok |= kb[kj * 4 + r] != 0 ? bit : 0u;
        }
}

// operands from [rows][D] tensors in global memory (rows past T read as zeros)
struct BertGlobalLd {
    const float* qp; const float* kp; const float* vp; long long rowbase; int T, D;
    __device__ __forceinline__ float4 q(int row, int col) const { return ld4_row(qp, rowbase, row, T, D, col); }
    __device__ __forceinline__ float4 k(int row, int col) const { return ld4_row(kp, rowbase, row, T, D, col); }
    __device__ __forceinline__ float4 v(int row, int col) const { return ld4_row(vp, rowbase, row, T, D, col); }
};

// head h's K as row fragments; V^T (lane (m, g): key 16 kj + 4 g + r, dim 16 c + m) from V's row fragments by a 16 x 16 transpose through the
// wave's LDS tile -- as loads the transposed fragments were 32 four-byte requests per lane, each touching four 64-byte segments
template <class Ld>
__device__ __forceinline__ void bert_kv_frags(const Ld& ld, int h, float* __restrict__ tile, float4 (&kf)[4][2], float (&vt)[4][4][2]) {
    const int lane = lane_id(), m = lane & 15, gq = lane >> 4;
    float4 vf[4][2];
#pragma unroll
    for (int kj = 0; kj < 4; ++kj)
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            kf[kj][c] = ld.k(kj * 16 + m, h * BHD + 16 * c + 4 * gq);
            vf[kj][c] = ld.v(kj * 16 + m, h * BHD + 16 * c + 4 * gq);
        }
#pragma unroll
    for (int kj = 0; kj < 4; ++kj)
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            float t4[4];
            tile_transpose(tile, vf[kj][c], t4);
#pragma unroll
            for (int r = 0; r < 4; ++r) vt[kj][r][c] = t4[r];
        }
}

// one query tile of one head: qraw = the tile's unscaled q fragments (lane (m, g): row m, dims 16 c + 4 g ..), kw = the row's dropout keep
// word (all ones outside training), NT = ceil(T / 16).  ov[c] = the normalised output of dims 16 c + 4 g .. of row m; mx, rl = the row's
// softmax statistics (max, 1 / sum)
__device__ __forceinline__ void bert_attn_qtile(const float4 (&kf)[4][2], const float (&vt)[4][4][2], const float4 (&qraw)[2], float inv, int NT,
                                                unsigned valid, unsigned okb, unsigned long long kw, float dscale, float4 (&ov)[2], float& mx_out,
                                                float& rl_out) {
    const int gq = lane_id() >> 4;
    float4 qf[2];
#pragma unroll
    for (int c = 0; c < 2; ++c) qf[c] = f4scale(qraw[c], inv);
    f32x4 s[4];
    float mx = -INFINITY;
#pragma unroll
    for (int kj = 0; kj < 4; ++kj) {
        s[kj] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (kj < NT) {
            s[kj] = frag2(kf[kj], qf, s[kj]);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const unsigned bit = 1u << (kj * 4 + r);
                s[kj][r] = !(valid & bit) ? -INFINITY : ((okb & bit) ? s[kj][r] : -1e9f);
                mx = fmaxf(mx, s[kj][r]);
            }
        }
    }
    mx = quad_group_max(mx);
    float l = 0.f;
    f32x4 oacc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
    for (int kj = 0; kj < 4; ++kj) {
        if (kj < NT) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int n = kj * 16 + 4 * gq + r;
                const float p = fast_exp(s[kj][r] - mx);
                l += p;
                const float pd = ((kw >> n) & 1ull) ? p * dscale : 0.f;
                oacc[0] = mfma4(vt[kj][r][0], pd, oacc[0]);
                oacc[1] = mfma4(vt[kj][r][1], pd, oacc[1]);
            }
        }
    }
    l = quad_group_sum(l);
    const float rl = 1.0f / l;
#pragma unroll
    for (int c = 0; c < 2; ++c) ov[c] = make_float4(oacc[c][0] * rl, oacc[c][1] * rl, oacc[c][2] * rl, oacc[c][3] * rl);
    mx_out = mx; rl_out = rl;
}

}  // namespace amid
