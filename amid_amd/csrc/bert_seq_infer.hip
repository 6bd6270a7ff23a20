// BERT4Rec's inference encoder as ONE launch (evaluation: engine_bert.py _enqueue_eval_encoders): a workgroup per LIVE sequence gathers the
// sequence's T <= 64 rows from the item table, runs both TransformerBlocks in eval mode (model_seq.py:242-245: LNb_in -> q, k, v ->
// bidirectional masked attention over 4 heads of 32 -> out-projection + residual -> LNb_out -> 4 x (W1 chunk, tanh GELU, W2 chunk) +
// residual; no dropout: no Philox draws, the sites multiply by the runtime scale 1) and writes the last block's output rows -- nothing else: no y, q, k, v, o, stats, x1, y2, pre,
// h, no key mask bytes.  What the staged evaluation runs as six launches (gather, q / k / v strips, 2 x (attention core + out-projection /
// feed-forward strips)) with q, k, v, o and the block input going through HBM between them.
//
// Four waves, a wave owns the 16-row strip 16 w .. 16 w + 15 of the sequence and all 128 columns (rows past T are zeros nobody reads).
// The chain bodies are bert_strip_parts.h's (MODE 3: RingP3<128>, strip_mma16x6 on the three-plane tile images amid_bert_weight_images_f32
// wrote) and the attention core per (query tile, head) is attention_bert_parts.h's: every row gets the bits the strip launches give it.
// LDS: the ring's four 32 KB slabs + 8 KB (the waves' transpose tiles).  Between v's product and the out-projection the chain has ENDED:
// the ring's mid / lo slots are idle and take the sequence's K and V images ([64 keys][128] fp32, 16-byte chunk c of row n at chunk
// position c ^ (n & 15): conflict-free fragment reads), Wo's hi plane lands in the idle hi slot under the attention core, its mid / lo
// planes are requested when the core is done with the images (RingP3::restart_hi / restart_ml).
#include "common.h"
#include "bert_strip_parts.h"
#include "attention_bert_parts.h"

namespace amid {

struct BSeqInferArgs {
    BStripQkvArgs q[2];          // per block (the saved-tensor fields are unused)
    BStripOffArgs f[2];
    float* x_out;                // [2, B, T, 128]
    const float* table; long long n_rows; const int* idx; const long long* seq_d2; const int* live;
    int B, T;
    float att_scale;
};

// operands of the attention core from the K / V images in LDS (rows past T read as zeros) and the wave's q strip
struct BertLdsLd {
    const float* kimg; const float* vimg; int T;
    __device__ __forceinline__ float4 at(const float* img, int row, int col) const {
        const float4 v = ld4(img + row * BSD + 4 * ((col >> 2) ^ (row & 15)));
        return (row < T) ? v : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    __device__ __forceinline__ float4 k(int row, int col) const { return at(kimg, row, col); }
    __device__ __forceinline__ float4 v(int row, int col) const { return at(vimg, row, col); }
};
__device__ __forceinline__ void strip_to_image(float* __restrict__ img, const StripRegs<BSD>& x) {
    const int lane = lane_id(), m = lane & 15, g = lane >> 4;
    float* rowp = img + (wave_id() * 16 + m) * BSD;
#pragma unroll
    for (int ct = 0; ct < BNT; ++ct) st4(rowp + 4 * ((4 * ct + g) ^ m), make_float4(x.v[ct][0], x.v[ct][1], x.v[ct][2], x.v[ct][3]));
}
// key_bits (attention_bert_parts.h) straight from the sequence's ids: visible = seq_d2 > 0 (model_seq.py:288)
__device__ __forceinline__ void key_bits_seq(const long long* __restrict__ sq, int T, int gq, unsigned& valid, unsigned& ok) {
    long long id[16];
#pragma unroll
    for (int kj = 0; kj < 4; ++kj)
#pragma unroll
        for (int r = 0; r < 4; ++r) id[kj * 4 + r] = sq[min(kj * 16 + 4 * gq + r, T - 1)];
    valid = 0; ok = 0;
#pragma unroll
    for (int kj = 0; kj < 4; ++kj)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int n = kj * 16 + 4 * gq + r;
            const unsigned bit = n < T ? 1u << (kj * 4 + r) : 0u;
            valid |= bit;
            ok |= id[kj * 4 + r] > 0 ? bit : 0u;
        }
}

__global__ __launch_bounds__(STRIP_THREADS) void bert_seq_infer_kernel(const BSeqInferArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    using R = RingP3<BSD>;
    const int T = a.T, B = a.B;
    const int j = blockIdx.x;
    const int n0 = a.live[B];
    const int g = j >= n0 ? 1 : 0, b = a.live[j];          // bert_live_seq's order
    R ring(smem);
    ring.first(a.q[0].w[0][g]);
    const int lane = lane_id(), m = lane & 15, gq = lane >> 4, w = wave_id();
    const int NT = (T + 15) >> 4;
    // the strip's geometry: this lane's row t of sequence (g, b); only x_out is ever stored through it
    StripGeom sg;
    sg.M = B * T; sg.B = B; sg.T = T; sg.act_bytes = (unsigned)(2LL * B * T * BSD * 4); sg.tm_bytes = sg.act_bytes / 16; sg.tpg = 0; sg.live = nullptr;
    const int t = w * 16 + m;
    StripRow row;
    row.ok = t < T;
    row.local = b * T + (row.ok ? t : 0);
    row.off = row.ok ? ((unsigned)g * (unsigned)sg.M + (unsigned)row.local) * (unsigned)(BSD * 4) + 16u * (unsigned)gq : STRIP_OOB;
    // the gather: x = table[idx[g][b][t]] (no positional table, no dropout: engine_bert.py enqueue_forward); ids were validated by the marshal
    StripRegs<BSD> X;
    {
        long long id = a.idx[(long long)g * sg.M + (long long)b * T + min(t, T - 1)];
        id = id < 0 ? 0 : (id >= a.n_rows ? a.n_rows - 1 : id);
        const float* src = a.table + id * BSD + 4 * gq;
#pragma unroll
        for (int ct = 0; ct < BNT; ++ct) {
            const f32x4 v = __builtin_nontemporal_load((const f32x4*)(src + 16 * ct));
            X.v[ct] = row.ok ? v : f32x4{0.f, 0.f, 0.f, 0.f};
        }
    }
    unsigned valid, okb;
    key_bits_seq(a.seq_d2 + (long long)b * T, T, gq, valid, okb);
    const float inv = 1.0f / a.att_scale;
    float* kimg = ring.mslot();
    float* vimg = ring.lslot();
    float* tile = smem + 4 * R::SLAB + w * ATTN_BWD_TILE_FLOATS;
    const BertLdsLd ld{kimg, vimg, T};
    ColVec<BSD> la, lb;
    la.load(a.q[0].la[g]); lb.load(a.q[0].lb[g]);
    static_for<2>([&](auto LL) {
        constexpr int l = decltype(LL)::value;
        StripRegs<BSD> Q, K, V, O;
        bqkv_fwd_chain<false, false>(a.q[l], sg, ring, row, g, X, la, lb, Q, K, V);
        // every wave is past v's mid barrier: the mid / lo slots and the other hi slot are idle
        ring.restart_hi(a.f[l].wo[g]);
        strip_to_image(kimg, K);
        strip_to_image(vimg, V);
        __syncthreads();
#pragma unroll
        for (int h = 0; h < 4; ++h) {
            float4 ov[2] = {make_float4(0.f, 0.f, 0.f, 0.f), make_float4(0.f, 0.f, 0.f, 0.f)};
            if (w < NT) {                                   // (wave-uniform: a strip past T has no query)
                float4 kf[4][2];
                float vt[4][4][2];
                bert_kv_frags(ld, h, tile, kf, vt);
                float4 qraw[2];
#pragma unroll
                for (int c = 0; c < 2; ++c) qraw[c] = make_float4(Q.v[2 * h + c][0], Q.v[2 * h + c][1], Q.v[2 * h + c][2], Q.v[2 * h + c][3]);
                float mx, rl;
                bert_attn_qtile(kf, vt, qraw, inv, NT, valid, okb, ~0ull, 1.0f, ov, mx, rl);
            }
#pragma unroll
            for (int c = 0; c < 2; ++c) O.v[2 * h + c] = f32x4{ov[c].x, ov[c].y, ov[c].z, ov[c].w};
        }
        __syncthreads();                                    // everybody is done with the images
        ring.restart_ml();
        boff_fwd_chain<l == 0, false, false>(a.f[l], a.q[1], sg, ring, row, g, O, X, la, lb);
        X = O;
    });
    strip_store<BSD>(GBuf(a.x_out, sg.act_bytes), row, X);
}

}  // namespace amid

using namespace amid;
using namespace amid_strip_host;

// 1 when the one-launch inference encoder covers the shape: hidden 128, 4 heads, T <= 64 (a workgroup holds the sequence)
extern "C" int amid_bert_seq_infer_supported(int B, int T, int D, int H) {
    return (D == BSD && H == 4 && T > 0 && T <= 64 && B > 0) ? 1 : 0;
}

// Parameter arrays are host arrays of device pointers ordered [block][domain] (4 entries); w3_img / b3 [block][q, k, v][domain] (12 entries).
// Every weight is a three-plane tile image of amid_bert_weight_images_f32 (w1_img / w2_img: the first of the four tiles' images, one
// behind the other), as the *_p3_f32 strip entry points take them.
extern "C" int amid_bert_seq_fwd_gather_infer_f32(float* x_out, const float* const* la1, const float* const* lb1, const float* const* w3_img,
                                                  const float* const* b3, const float* const* wo_img, const float* const* bo,
                                                  const float* const* la2, const float* const* lb2, const float* const* w1_img,
                                                  const float* const* b1, const float* const* w2_img, const float* const* b2, int B, int T,
                                                  const int* live, const float* table, long long n_rows, const int* idx_all,
                                                  const long long* seq_d2, void* stream) {
    AMID_CHECK_ARG(x_out && la1 && lb1 && w3_img && b3 && wo_img && bo && la2 && lb2 && w1_img && b1 && w2_img && b2 && live && table && idx_all &&
                   seq_d2 && n_rows > 0 && B > 0 && T > 0);
    if (!amid_bert_seq_infer_supported(B, T, BSD, 4)) return AMID_ERR_UNSUPPORTED;
    BSeqInferArgs a = {};
    for (int l = 0; l < 2; ++l)
        for (int g = 0; g < 2; ++g) {
            const int i = 2 * l + g;
            AMID_CHECK_ARG(la1[i] && lb1[i] && wo_img[i] && bo[i] && la2[i] && lb2[i] && w1_img[i] && b1[i] && w2_img[i] && b2[i]);
            a.q[l].la[g] = la1[i]; a.q[l].lb[g] = lb1[i];
            for (int k = 0; k < 3; ++k) {
                const int i3 = (3 * l + k) * 2 + g;
                AMID_CHECK_ARG(w3_img[i3] && b3[i3]);
                a.q[l].w[k][g] = w3_img[i3]; a.q[l].b[k][g] = b3[i3];
            }
            a.f[l].wo[g] = wo_img[i]; a.f[l].bo[g] = bo[i]; a.f[l].la[g] = la2[i]; a.f[l].lb[g] = lb2[i];
            a.f[l].w1[g] = w1_img[i]; a.f[l].b1[g] = b1[i]; a.f[l].w2[g] = w2_img[i]; a.f[l].b2[g] = b2[i];
            a.f[l].layer = l; a.f[l].train = 0; a.f[l].spec = 0u; a.f[l].scale = 1.0f;
        }
    if (2LL * B * T * BSD * 4 > 0x7FFFFFF0LL) return AMID_ERR_UNSUPPORTED;      // the [2, B, T, 128] output goes through a buffer descriptor: 2 GiB
    a.x_out = x_out; a.table = table; a.n_rows = n_rows; a.idx = idx_all; a.seq_d2 = seq_d2; a.live = live; a.B = B; a.T = T;
    a.att_scale = sqrtf((float)(BSD / 4));                                  // attention.hip attn_fill: sqrt(d_k) for the bidirectional core
    return launch_lds<bert_seq_infer_kernel>(B, STRIP_THREADS, strip_lds_bytes<BSD>(), stream, a);
}
