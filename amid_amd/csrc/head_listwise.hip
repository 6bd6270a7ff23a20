// The scorer of a train step under a LISTWISE objective on K sampled negatives, one launch, one workgroup per batch row b:
//   scorer forward over the row's NI = 1 + K candidates (predictModule.forward, model_seq.py:40-54; the positive is column 0,
//   dataset_seq.py:191,199)  ->  the row's objective on the own domain's LOGITS (sampled softmax or BPR; the reference's mask zeroes the
//   other domain, train_sr.py:205-211)  ->  scorer backward from dLoss/dz.
// It is the one-head form of scorer_multi_fwd_bwd_kernel (head_fused.hip) with another middle: W1^T staged in LDS, the user vectors
// u [2, B, D] given, items in chunks of 64, the same transpose riders on the extra workgroups (blockIdx >= B), so it takes that launch's
// place in a step.  The masked BCE's backward starts from dLoss/dp and multiplies by p (1 - p); a listwise gradient sent through p would
// be divided by p (1 - p) first, which is 0 once p rounds to 1.0f.  Here the gradient never leaves the logits: the backward
// (scorer_bwd_part<.., DZ = true>) takes dLoss/dz as it is.
//
// Summation order (every sum of the objective, and the maximum): thread t of the 512 takes the candidates n = t and n = t + 512 in that
// order (NI <= 1024), the 64 lanes of a wave are joined by group_sum<64> / group_max<64> (common.h's balanced tree in lane order), and the
// eight waves' values w0 .. w7 as ((w0 + w1) + (w2 + w3)) + ((w4 + w5) + (w6 + w7)).  Nothing is accumulated atomically: the same inputs
// give the same bits.
//   kind 1, softmax:  m = max_n z[n],  lse = m + log sum_n exp(z[n] - m),  L = lse - z[0],  dz[n] = exp(z[n] - lse) - [n == 0]
//   kind 2, BPR:      K = NI - 1,  x_n = z[n] - z[0],  L = (1 / K) sum_{n >= 1} (max(x_n, 0) + log1p(exp(-|x_n|))),
//                     dz[n] = sigmoid(x_n) / K (n >= 1),  dz[0] = -sum_{n >= 1} dz[n]
//   both:             loss_part[b] = L / B,  dz / B leaves in dz1 / dz2 (the other domain's: 0)
#include "head_listwise_parts.h"

namespace amid {

__global__ __launch_bounds__(512) void scorer_listwise_fwd_bwd_kernel(const ListwiseArgs m) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const HeadArgs& a = m.h;
    if ((int)blockIdx.x >= a.B) { transpose_extra(a, sm); return; }
    const int b = blockIdx.x, D = a.D;
    const Tg tg = whole_block();
    const size_t carve = head_carve_floats(D, a.hid, 64);
    HeadLds s(sm, D, a.hid, 64);
    float* zs = sm + carve;                                    // [LW_MAX_NI] the own domain's logits
    float* red = zs + LW_MAX_NI;                               // [8]
    s.scr = red;
    const int own = a.domain[b] != 0 ? 1 : 0;
    stage_w1t(s.w1t, a.w1, 2 * D, a.hid, tg);
    for (int e = tg.tid; e < 2 * D; e += tg.n) s.u_s[e] = a.u[((long long)(e / D) * a.B + b) * D + (e % D)];
    __syncthreads();
    listwise_fwd_part(a, s, b, own, zs, tg);
    listwise_objective(a, m.kind, b, own, zs, red);
    __threadfence_block();                                     // dz written above is read by other threads of this workgroup below
    __syncthreads();
    scorer_bwd_part<true, false, true>(a, s, b, tg);           // ends with a barrier; d u left at the start of the ci region
    for (int e = threadIdx.x; e < 2 * D; e += blockDim.x) m.du[((long long)(e / D) * a.B + b) * D + (e % D)] = s.ci[e];
}

}  // namespace amid

using namespace amid;

// Scorer forward + listwise objective + scorer backward in ONE launch on given user vectors u [2, B, D] and candidate rows items
// [B, NI, D] (column 0: the positive; no labels are read).  kind 1: sampled softmax, 2: BPR -- on the logits of the row's own domain
// (domain_id[b] != 0).  Outputs: p1 / p2 [B, NI] (the bits of amid_scorer_fwd_f32), loss_part [B] (L_b / B), dz1 / dz2 [B, NI]
// (dLoss/dz; the other domain's 0), du [2, B, D] (the other domain's half 0), ditems [B, NI, D], sc_part (per-row partials of dW1, db1,
// dW2, db2: amid_scorer_part_floats a row).  tr_src / tr_dst / n_tr: the transposes the extra workgroups do, as amid_head_bwd_f32's.
extern "C" int amid_scorer_listwise_fwd_bwd_f32(const float* u, const float* items, const float* w1, const float* b1, const float* w2,
                                                const float* b2, const long long* domain_id, int kind, int B, int NI, int D, int hid,
                                                float* p1, float* p2, float* dz1, float* dz2, float* loss_part, float* du, float* ditems,
                                                float* sc_part, const float* const* tr_src, float* const* tr_dst, int n_tr, void* stream) {
    AMID_CHECK_ARG(u && items && w1 && b1 && w2 && b2 && domain_id && p1 && p2 && dz1 && dz2 && loss_part && du && ditems && sc_part);
    AMID_CHECK_ARG((kind == 1 || kind == 2) && B > 0 && NI >= 2 && D > 0 && n_tr >= 0 && n_tr <= 32);
    for (int i = 0; i < n_tr; ++i) AMID_CHECK_ARG(tr_src && tr_dst && tr_src[i] && tr_dst[i]);
    if (NI > LW_MAX_NI || D > 128 || (D % 32) != 0 || hid <= 0 || hid > 64 || (hid % 4) != 0) return AMID_ERR_UNSUPPORTED;
    ListwiseArgs m = {};
    HeadArgs& a = m.h;
    a.x = u; a.items = items; a.w1 = w1; a.b1 = b1; a.w2 = w2; a.b2 = b2; a.domain = domain_id;
    a.B = B; a.T = 1; a.NI = NI; a.D = D; a.hid = hid; a.eps = 0.f;
    a.u = const_cast<float*>(u); a.p1 = p1; a.p2 = p2; a.dp1 = dz1; a.dp2 = dz2; a.loss_part = loss_part; a.ditems = ditems; a.sc_part = sc_part;
    a.n_tr = n_tr;
    for (int i = 0; i < n_tr; ++i) { a.tr_src[i] = tr_src[i]; a.tr_dst[i] = tr_dst[i]; }
    m.kind = kind; m.du = du;
    const size_t lds = (head_carve_floats(D, hid, 64) + LW_MAX_NI + 8) * sizeof(float);
    if (lds > 160 * 1024) return AMID_ERR_UNSUPPORTED;
    if (lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute((const void*)scorer_listwise_fwd_bwd_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return (int)e;
    }
    const int extra = n_tr > 0 ? min(n_tr * (D / 32) * (D / 32), 96) : 0;
    scorer_listwise_fwd_bwd_kernel<<<B + extra, 512, lds, (hipStream_t)stream>>>(m);
    AMID_LAUNCH_CHECK();
    return AMID_OK;
}
