// Hard-negative mining inside the listwise launch: one workgroup of 512 threads per batch row b
//   scorer forward over ALL of the row's NI = 1 + M candidates (listwise_fwd_part: p1 / p2, the own domain's logits zs [NI] in LDS)
//   ->  selection in LDS: of the M negatives the H ranked S .. S + H - 1 by logit are kept (a higher logit ranks first, ties go to the
//       lower position), the compact list c = [0] + kept positions ascending, NC = 1 + H entries
//   ->  the row's objective (head_listwise.hip's formulas) on z[c], NI -> NC
//   ->  scorer backward over the compact list ONLY, in chunks of 64 list entries: the backward's work scales with 1 + H, not NI;
//       the d items rows of the candidates that were not kept are cleared with plain vector stores.
// Selection is a constant for differentiation (as torch.topk's indices are): no gradient flows through it.
//
// Rank by counting: rank(n) = #{ j in 1 .. M : z[j] > z[n] or (z[j] == z[n] and j < n) } -- thread t ranks the positions t and t + 512
// against every negative read from LDS (one broadcast read a compare pair); no sort.  With finite logits the ranks are a permutation of
// 0 .. M - 1, so exactly H negatives are kept.  The list is built by a ballot per wave and the prefix of the waves' counts: ascending by
// construction (lane order inside a wave, waves in order, the pass over t before the pass over t + 512).
//
// Summation order of the objective: head_listwise.hip's over LIST ENTRIES -- thread t takes the entries t and t + 512, group_sum<64> /
// group_max<64> inside a wave, the eight waves as ((w0 + w1) + (w2 + w3)) + ((w4 + w5) + (w6 + w7)).  The backward walks the list in order
// (hidden unit j sums over the entries of a chunk in list order, chunk after chunk; the item half of dW1 accumulates over the chunks).
// Nothing is accumulated atomically: the same inputs give the same bits.  At H = M, S = 0 the list is 0 .. NI - 1 and p, z, the loss and
// dz are the listwise launch's bits.
#include "head_listwise_parts.h"

namespace amid {

struct MinedArgs {
    ListwiseArgs l;
    int keep, skip;            // H, S
    int* sel;                  // [B, keep] the kept positions, ascending
    float* z;                  // [B, NI] the own domain's logits
};

#pragma clang fp contract(off)

// the objective of listwise_objective on the list's logits zs[list[i]], i < NC: loss_part[b], and dz / B per list entry into dzc [NC]
__device__ __forceinline__ void mined_objective(const HeadArgs& a, int kind, int b, int NC, const float* __restrict__ zs,
                                                const int* __restrict__ list, float* __restrict__ dzc, float* __restrict__ red) {
    const int t = threadIdx.x;
    const float fB = (float)a.B;
    const float z0 = zs[0];
    if (kind == 1) {
        float m = -INFINITY;
        for (int i = t; i < NC; i += 512) m = fmaxf(m, zs[list[i]]);
        m = lw_block_max(m, red);
        float e = 0.f;
        for (int i = t; i < NC; i += 512) e += expf(zs[list[i]] - m);
        const float lse = m + logf(lw_block_sum(e, red));
        for (int i = t; i < NC; i += 512) dzc[i] = (expf(zs[list[i]] - lse) - (i == 0 ? 1.f : 0.f)) / fB;
        if (t == 0) a.loss_part[b] = (lse - z0) / fB;
    } else {
        const float fK = (float)(NC - 1);
        float l = 0.f, g = 0.f;
        for (int i = t; i < NC; i += 512) {
            if (i == 0) continue;
            const float x = zs[list[i]] - z0;
            l += fmaxf(x, 0.f) + log1pf(expf(-fabsf(x)));
            const float gn = (1.0f / (1.0f + expf(-x))) / fK;
            g += gn;
            dzc[i] = gn / fB;
        }
        l = lw_block_sum(l, red);
        g = lw_block_sum(g, red);
        if (t == 0) { dzc[0] = -g / fB; a.loss_part[b] = (l / fK) / fB; }
    }
}

// item_half for the list entries i0 .. i0 + nn: ci[n][j] = sum_e w1t[D+e][j] item[list[i0 + n]][e]
__device__ __forceinline__ void item_half_list(const HeadArgs& a, const HeadLds& s, int b, const int* __restrict__ list, int i0, int nn, const Tg tg) {
    const int D = a.D, hid = a.hid;
    const int part = tg.tid & 7;
    for (int o0 = 0; o0 < nn * hid; o0 += tg.n >> 3) {
        const int nj = o0 + (tg.tid >> 3);
        const bool on = nj < nn * hid;
        const int n = on ? nj / hid : 0, j = on ? nj - n * hid : 0;
        float acc = 0.f;
        if (on) acc = item_half_chain(s.w1t + D * (hid + 1) + j, hid + 1, a.items + ((long long)b * a.NI + list[i0 + n]) * D, D, part);
        acc = group_sum<8>(acc);
        if (on && part == 0) s.ci[n * (hid + 1) + j] = acc;
    }
}

// scorer_bwd_part<FUSED, .., DZ> over the compact list: dz of the own domain per list entry in dzc (the other domain's is 0), W1^T, the
// user vectors and their pre-activations (s.w1t, s.u_s, s.au) still in LDS from the forward.  d u [2][D] is left at the start of s.ci.
__device__ __forceinline__ void mined_bwd_part(const HeadArgs& a, const HeadLds& s, int b, int own, int NC, const int* __restrict__ list,
                                               const float* __restrict__ dzc, const Tg tg) {
    const int D = a.D, hid = a.hid, NI = a.NI;
    const int P = (hid * 2 * D + 2 * hid + 1 + 3) & ~3;      // amid_scorer_part_floats
    float* part = a.sc_part + (long long)b * P;
    for (int e = tg.tid; e < 2 * hid; e += tg.n) s.da[e] = 0.f;
    for (int e = tg.tid; e < hid + 1; e += tg.n) s.dw2[e] = 0.f;
    const int CH = s.chunk;
    for (int i0 = 0; i0 < NC; i0 += CH) {
        const int nn = min(CH, NC - i0);
        __syncthreads();
        item_half_list(a, s, b, list, i0, nn, tg);
        __syncthreads();
        if (tg.tid < hid) {                       // hidden unit j walks the chunk's list entries in order
            const int j = tg.tid;
            float s_da0 = 0.f, s_da1 = 0.f, s_w2 = 0.f;
            const float w2j = a.w2[j];
            for (int n = 0; n < nn; ++n) {
                const float dzo = dzc[i0 + n];
                const float dz1 = own ? 0.f : dzo, dz2 = own ? dzo : 0.f;
                const float c = s.ci[n * (hid + 1) + j];
                const float h1 = fmaxf(s.au[j] + c, 0.f), h2 = fmaxf(s.au[hid + j] + c, 0.f);
                const float g1 = h1 > 0.f ? dz1 * w2j : 0.f, g2 = h2 > 0.f ? dz2 * w2j : 0.f;
                s_w2 += dz1 * h1 + dz2 * h2;
                s_da0 += g1; s_da1 += g2;
                s.dc[n * (hid + 1) + j] = g1 + g2;
            }
            s.da[j] += s_da0; s.da[hid + j] += s_da1; s.dw2[j] += s_w2;
        }
        if (tg.tid == 64) {
            float acc = 0.f;
            for (int n = 0; n < nn; ++n) acc += dzc[i0 + n];
            s.dw2[hid] += acc;
        }
        __syncthreads();
        // d item[list[i]][e] = sum_j dc[n][j] w1t[D+e][j]
        for (int ne = tg.tid; ne < nn * D; ne += tg.n) {
            const int n = ne / D, e = ne - n * D;
            float acc = 0.f;
            const float* wp = s.w1t + (D + e) * (hid + 1);
#pragma unroll 8
            for (int j = 0; j < hid; ++j) acc = fmaf(s.dc[n * (hid + 1) + j], wp[j], acc);
            a.ditems[((long long)b * NI + list[i0 + n]) * D + e] = acc;
        }
        // dW1[j][D+e] (+)= sum_n dc[n][j] item[list[i]][e]  (thread tid owns the same (j, e) in every chunk)
        for (int je = tg.tid; je < hid * D; je += tg.n) {
            const int j = je / D, e = je - j * D;
            float acc = 0.f;
            for (int n = 0; n < nn; ++n) acc = fmaf(s.dc[n * (hid + 1) + j], a.items[((long long)b * NI + list[i0 + n]) * D + e], acc);
            float* dst = part + j * 2 * D + D + e;
            *dst = (i0 == 0) ? acc : *dst + acc;
        }
    }
    __syncthreads();
    float* du_s = s.ci;
    for (int de = tg.tid; de < 2 * D; de += tg.n) {
        const int d = de / D, e = de - d * D;
        float acc = 0.f;
        const float* wp = s.w1t + e * (hid + 1);
#pragma unroll 8
        for (int j = 0; j < hid; ++j) acc = fmaf(s.da[d * hid + j], wp[j], acc);
        du_s[de] = acc;
    }
    for (int je = tg.tid; je < hid * D; je += tg.n) {
        const int j = je / D, e = je - j * D;
        part[j * 2 * D + e] = s.da[j] * s.u_s[e] + s.da[hid + j] * s.u_s[D + e];
    }
    for (int j = tg.tid; j < hid; j += tg.n) {
        part[hid * 2 * D + j] = s.da[j] + s.da[hid + j];            // db1
        part[hid * 2 * D + hid + j] = s.dw2[j];                     // dW2
    }
    if (tg.tid == 0) part[hid * 2 * D + 2 * hid] = s.dw2[hid];   // db2
    __syncthreads();
}

#pragma clang fp contract(fast)

// LDS behind the head's carve: zs [1024] | red [8] | dzc [1024] | list [1024] | inv [1024] | wcnt [16]
constexpr int MINED_EXTRA_FLOATS = 4 * LW_MAX_NI + 8 + 16;

__global__ __launch_bounds__(512) void scorer_mined_fwd_bwd_kernel(const MinedArgs m) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const HeadArgs& a = m.l.h;
    if ((int)blockIdx.x >= a.B) { transpose_extra(a, sm); return; }
    const int b = blockIdx.x, D = a.D, NI = a.NI, t = threadIdx.x;
    const int H = m.keep, S = m.skip, NC = 1 + H;
    const Tg tg = whole_block();
    const size_t carve = head_carve_floats(D, a.hid, 64);
    HeadLds s(sm, D, a.hid, 64);
    float* zs = sm + carve;                                    // [LW_MAX_NI] the own domain's logits
    float* red = zs + LW_MAX_NI;                               // [8]
    float* dzc = red + 8;                                      // [LW_MAX_NI] dz / B per list entry
    int* list = reinterpret_cast<int*>(dzc + LW_MAX_NI);       // [LW_MAX_NI] list entry -> position
    int* inv = list + LW_MAX_NI;                               // [LW_MAX_NI] position -> list entry, -1: not kept
    int* wcnt = inv + LW_MAX_NI;                               // [2][8] kept positions per (pass, wave)
    s.scr = red;
    const int own = a.domain[b] != 0 ? 1 : 0;
    stage_w1t(s.w1t, a.w1, 2 * D, a.hid, tg);
    for (int e = tg.tid; e < 2 * D; e += tg.n) s.u_s[e] = a.u[((long long)(e / D) * a.B + b) * D + (e % D)];
    __syncthreads();
    listwise_fwd_part(a, s, b, own, zs, tg);                   // ends with a barrier
    // ---- selection: ranks by counting, position 0 (the positive) always in the list
    const int n0 = t, n1 = t + 512;
    const float za = n0 < NI ? zs[n0] : 0.f, zb = n1 < NI ? zs[n1] : 0.f;
    int ra = 0, rb = 0;
    for (int j = 1; j < NI; ++j) {
        const float zj = zs[j];
        ra += (zj > za || (zj == za && j < n0)) ? 1 : 0;
        rb += (zj > zb || (zj == zb && j < n1)) ? 1 : 0;
    }
    const bool ka = n0 == 0 || (n0 < NI && ra >= S && ra < S + H);
    const bool kb = n1 < NI && rb >= S && rb < S + H;
    const unsigned long long ba = __ballot(ka), bb = __ballot(kb);
    const unsigned long long below = (1ull << lane_id()) - 1ull;
    const int w = wave_id();
    if (lane_id() == 0) { wcnt[w] = __popcll(ba); wcnt[8 + w] = __popcll(bb); }
    for (int n = t; n < NI; n += 512) m.z[(long long)b * NI + n] = zs[n];
    for (int i = t; i < NC; i += 512) list[i] = 0;             // (every entry a valid position whatever the logits)
    __syncthreads();
    int offa = 0, offb = 0;
    for (int k = 0; k < 8; ++k) { offa += k < w ? wcnt[k] : 0; offb += wcnt[k] + (k < w ? wcnt[8 + k] : 0); }
    const int ia = offa + __popcll(ba & below), ib = offb + __popcll(bb & below);
    // (finite logits: exactly NC entries; the bounds keep a row with NaN logits -- outside the contract -- inside the arrays)
    if (n0 < NI) inv[n0] = ka && ia < NC ? ia : -1;
    if (n1 < NI) inv[n1] = kb && ib < NC ? ib : -1;
    if (ka && ia < NC) list[ia] = n0;
    if (kb && ib < NC) list[ib] = n1;
    __syncthreads();
    for (int i = t; i < H; i += 512) m.sel[(long long)b * H + i] = list[1 + i];
    // ---- the objective on the list, dz rows, the d items rows of the candidates not kept
    mined_objective(a, m.l.kind, b, NC, zs, list, dzc, red);
    __syncthreads();
    float* dz_own = (own ? a.dp2 : a.dp1) + (long long)b * NI;
    float* dz_oth = (own ? a.dp1 : a.dp2) + (long long)b * NI;
    for (int n = t; n < NI; n += 512) { const int i = inv[n]; dz_own[n] = i >= 0 ? dzc[i] : 0.f; dz_oth[n] = 0.f; }
    const int q = D >> 2;
    float* dit = a.ditems + (long long)b * NI * D;
    for (int e = t; e < NI * q; e += 512)
        if (inv[e / q] < 0) st4(dit + 4 * (long long)e, make_float4(0.f, 0.f, 0.f, 0.f));
    // ---- backward over the list
    mined_bwd_part(a, s, b, own, NC, list, dzc, tg);           // ends with a barrier; d u left at the start of the ci region
    for (int e = threadIdx.x; e < 2 * D; e += blockDim.x) m.l.du[((long long)(e / D) * a.B + b) * D + (e % D)] = s.ci[e];
}

}  // namespace amid

using namespace amid;

// amid_scorer_listwise_fwd_bwd_f32 with hard-negative mining: of the row's NI - 1 negatives the `keep` ranked skip .. skip + keep - 1 by
// their own-domain logit enter the objective and the backward (the header's comment).  Further outputs: sel
// [B, keep] the kept positions ascending, z [B, NI] the own domain's logits.
extern "C" int amid_scorer_mined_fwd_bwd_f32(const float* u, const float* items, const float* w1, const float* b1, const float* w2,
                                             const float* b2, const long long* domain_id, int kind, int keep, int skip, int B, int NI, int D,
                                             int hid, float* p1, float* p2, float* dz1, float* dz2, float* loss_part, float* du, float* ditems,
                                             float* sc_part, int* sel, float* z, const float* const* tr_src, float* const* tr_dst, int n_tr,
                                             void* stream) {
    AMID_CHECK_ARG(u && items && w1 && b1 && w2 && b2 && domain_id && p1 && p2 && dz1 && dz2 && loss_part && du && ditems && sc_part);
    AMID_CHECK_ARG(sel && z);
    AMID_CHECK_ARG((kind == 1 || kind == 2) && B > 0 && NI >= 2 && D > 0 && n_tr >= 0 && n_tr <= 32);
    AMID_CHECK_ARG(keep >= 1 && skip >= 0 && (long long)skip + keep <= NI - 1);
    for (int i = 0; i < n_tr; ++i) AMID_CHECK_ARG(tr_src && tr_dst && tr_src[i] && tr_dst[i]);
    if (NI > LW_MAX_NI || D > 128 || (D % 32) != 0 || hid <= 0 || hid > 64 || (hid % 4) != 0) return AMID_ERR_UNSUPPORTED;
    MinedArgs m = {};
    HeadArgs& a = m.l.h;
    a.x = u; a.items = items; a.w1 = w1; a.b1 = b1; a.w2 = w2; a.b2 = b2; a.domain = domain_id;
    a.B = B; a.T = 1; a.NI = NI; a.D = D; a.hid = hid; a.eps = 0.f;
    a.u = const_cast<float*>(u); a.p1 = p1; a.p2 = p2; a.dp1 = dz1; a.dp2 = dz2; a.loss_part = loss_part; a.ditems = ditems; a.sc_part = sc_part;
    a.n_tr = n_tr;
    for (int i = 0; i < n_tr; ++i) { a.tr_src[i] = tr_src[i]; a.tr_dst[i] = tr_dst[i]; }
    m.l.kind = kind; m.l.du = du;
    m.keep = keep; m.skip = skip; m.sel = sel; m.z = z;
    const size_t lds = (head_carve_floats(D, hid, 64) + MINED_EXTRA_FLOATS) * sizeof(float);
    if (lds > 160 * 1024) return AMID_ERR_UNSUPPORTED;
    if (lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute((const void*)scorer_mined_fwd_bwd_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return (int)e;
    }
    const int extra = n_tr > 0 ? min(n_tr * (D / 32) * (D / 32), 96) : 0;
    scorer_mined_fwd_bwd_kernel<<<B + extra, 512, lds, (hipStream_t)stream>>>(m);
    AMID_LAUNCH_CHECK();
    return AMID_OK;
}
