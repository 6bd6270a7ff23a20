// The pieces of the BERT4Rec strip chains (bert_strip.hip) that more than one kernel file is built from: the weight ring of the fp32 builds,
// the reference LayerNorm on a strip, the dropout keep bits, the wide-tensor helpers, and the forward chain bodies -- LayerNorm + q / k / v,
// out-projection + feed-forward.  bert_strip.hip runs them a launch per chain over 64-row tiles and saves what the backward reads;
// bert_seq_infer.hip runs both blocks of a sequence in ONE launch and saves nothing.  A chain is row-independent, so both give a row the same bits.
#pragma once
#include "common.h"
#include "rng.h"
#include "strip_gemm.h"
#include "strip_chain.h"
#include "bert_math.h"

namespace amid {

constexpr int BSD = 128;            // hidden
constexpr int BSF = 512;            // feed-forward
constexpr int BSC = BSF / BSD;      // 128-column chunks of the feed-forward
constexpr int BNT = BSD / 16;

// strip_gemm.h's WDma for a tile whose rows lie LD floats apart in global memory (a column block of a wider matrix)
template <int D, int LD> struct WDmaLd {
    static constexpr int CPR = D / 4;
    static constexpr int PER_WAVE = D * CPR / 64 / STRIP_WAVES;
    static constexpr unsigned STRIDE2 = 2u * (256 / CPR) * LD * 4;
    unsigned off[2];
    int w;
    __device__ __forceinline__ WDmaLd() {
        const int lane = lane_id();
        w = wave_id();
#pragma unroll
        for (int k0 = 0; k0 < 2; ++k0) {
            const int p = (k0 * STRIP_WAVES + w) * 64 + lane;
            const int n = p / CPR, pos = p % CPR;
            off[k0] = (unsigned)((n * LD + ((pos ^ (n & 15)) * 4)) * 4);
        }
    }
    __device__ __forceinline__ void piece(float* __restrict__ buf, const float* __restrict__ W, int k0) const {
        const unsigned voff = off[k0 & 1] + (unsigned)(k0 >> 1) * STRIDE2;
        const unsigned lds = __builtin_amdgcn_readfirstlane(
            lds_offset(buf + (k0 * STRIP_WAVES + w) * 256));
        unsigned keep;
        asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 2\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
                     : "=&s"(keep) : "v"(voff), "s"(W), "s"(lds) : "memory");
    }
};

// the two-slab ring of strip_chain.h with a second source stride: fetch() takes a [128][128] tile with contiguous rows, fetch_ld() a
// column block of a [128][512] matrix
struct BRing {
    static constexpr bool BF16 = false;
    static constexpr int SLAB = BSD * BSD;
    float* buf; int s; WDma<BSD> dma; WDmaLd<BSD, BSF> dml;
    __device__ __forceinline__ explicit BRing(float* lds) : buf(lds), s(0) {}
    __device__ __forceinline__ void first(const float* __restrict__ W0) { dma.all(buf, W0); }
    __device__ __forceinline__ const float* next() {
        w_ring_wait();
        __syncthreads();
        const float* cur = buf + (s & 1) * SLAB;
        ++s;
        return cur;
    }
    static constexpr int SLOTS = 8 * BNT, EVERY = (SLOTS / 2) / WDma<BSD>::PER_WAVE;
    __device__ __forceinline__ void fetch(const float* __restrict__ W, int ct, int j) const {
        const int slot = ct * 8 + j;
        if (slot % EVERY == 0 && slot / EVERY < WDma<BSD>::PER_WAVE) dma.piece(buf + (s & 1) * SLAB, W, slot / EVERY);
    }
    __device__ __forceinline__ void fetch_ld(const float* __restrict__ W, int ct, int j) const {
        const int slot = ct * 8 + j;
        if (slot % EVERY == 0 && slot / EVERY < WDma<BSD>::PER_WAVE) dml.piece(buf + (s & 1) * SLAB, W, slot / EVERY);
    }
};

// MODE 3 (round 5): the products on bf16 pieces -- fp32 operands as hi + mid + lo, six piece pairs of v_mfma_f32_16x16x32_bf16, fp32
// accuracy (strip_gemm.h strip_mma16x6, strip_chain.h RingP3; what SASRec's strips run on since round 4).  Every 128 x 128 weight TILE
// the chains multiply with is then a three-plane fragment image (amid_bert_weight_images_f32): the weight arguments of the kernels point
// at images, a feed-forward weight at its four tiles' images one behind the other.
#ifndef AMID_BS_SPREAD
#define AMID_BS_SPREAD 1
#endif
constexpr bool BSPREAD = AMID_BS_SPREAD != 0;      // the hooks' slots between the piece products' matrix instructions (strip_gemm.h strip_mma16x6 SPREAD)
constexpr int BIMG = 3 * (BSD * BSD / 2);            // floats per tile image (three 32 KB planes)
template <int MODE> struct BRingSel { using type = BRing; };
template <> struct BRingSel<3> { using type = RingP3<BSD>; };
// tile c of a feed-forward weight whose tiles are ROW blocks of the fp32 matrix (w_1 [512][128], w_2^T [512][128]) ...
template <class R> __device__ __forceinline__ const float* btile_rows(const float* base, int c) {
    return base + (long long)c * (ring_is_p3<R>::value ? BIMG : BSD * BSD);
}
// ... and whose tiles are COLUMN blocks (w_2 [128][512], w_1^T [128][512]): fetched with the wide stride, or as the c-th image
template <class R> __device__ __forceinline__ void bfetch_cols(R& ring, const float* base, int c, int ct, int j) {
    if constexpr (ring_is_p3<R>::value) ring.fetch(base + (long long)c * BIMG, ct, j);
    else ring.fetch_ld(base + c * BSD, ct, j);
}

// ---- the reference LayerNorm on a strip: a (x - mean) / (std_unbiased + eps) + b -----------------------------------------------------
__device__ __forceinline__ void lnb_stats(const StripRegs<BSD>& x, float& mean, float& sd, float& r) {
    float s = 0.f;
#pragma unroll
    for (int ct = 0; ct < BNT; ++ct) s += (x.v[ct][0] + x.v[ct][1]) + (x.v[ct][2] + x.v[ct][3]);
    mean = row_sum4(s) * (1.0f / BSD);
    float q = 0.f;
#pragma unroll
    for (int ct = 0; ct < BNT; ++ct)
#pragma unroll
        for (int e = 0; e < 4; ++e) { const float d = x.v[ct][e] - mean; q = fmaf(d, d, q); }
    sd = sqrtf(row_sum4(q) * (1.0f / (BSD - 1)));
    r = 1.0f / (sd + BERT_EPS);
}
__device__ __forceinline__ void strip_lnb(StripRegs<BSD>& y, const StripRegs<BSD>& x, const ColVec<BSD>& a, const ColVec<BSD>& b) {
    float mean, sd, r;
    lnb_stats(x, mean, sd, r);
#pragma unroll
    for (int ct = 0; ct < BNT; ++ct)
#pragma unroll
        for (int e = 0; e < 4; ++e) y.v[ct][e] = a.v[ct][e] * (x.v[ct][e] - mean) * r + b.v[ct][e];
}
// backward: dx = r (g - mean(g)) - t r^2 xc / (std (D - 1)), g = a dy, t = sum(g xc); this lane's row adds dy xc r / dy to the column partials
__device__ __forceinline__ void strip_lnb_bwd(StripRegs<BSD>& dx, const StripRegs<BSD>& dy, const StripRegs<BSD>& x, const ColVec<BSD>& a,
                                              StripRegs<BSD>& dgam, StripRegs<BSD>& dbet) {
    float mean, sd, r;
    lnb_stats(x, mean, sd, r);
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int ct = 0; ct < BNT; ++ct)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float xc = x.v[ct][e] - mean;
            const float gg = a.v[ct][e] * dy.v[ct][e];
            s1 += gg;
            s2 = fmaf(gg, xc, s2);
            dgam.v[ct][e] = dy.v[ct][e] * xc * r;
            dbet.v[ct][e] = dy.v[ct][e];
            dx.v[ct][e] = gg;
        }
    const float gm = row_sum4(s1) * (1.0f / BSD);
    const float t = row_sum4(s2);
    const float c = (sd > 0.f) ? t * r * r / (sd * (BSD - 1)) : 0.f;
#pragma unroll
    for (int ct = 0; ct < BNT; ++ct)
#pragma unroll
        for (int e = 0; e < 4; ++e) dx.v[ct][e] = r * (dx.v[ct][e] - gm) - c * (x.v[ct][e] - mean);
}

// ---- dropout on a strip: the keep bits of this lane's 32 elements (bit 4 ct + e <-> column 16 ct + 4 g + e) -------------------------------
// p = 0.1 takes 16-bit decisions (rng.h): ONE Philox call decides 8 consecutive elements = the column quads of lanes (m, 2h) and
// (m, 2h + 1) of one column tile.  Lane (m, g) draws the calls of the column tiles ct with (ct & 1) == (g & 1), keeps its own quad's
// four decisions and hands the partner (lane ^ 16) the other four: four calls per lane and site instead of eight.  And the calls are
// drawn INSIDE the matrix loop in front of the epilogue that applies them, a round per MFMA group (slot()): the counters do not depend
// on data, a round is two quarter-rate multiplies + five plain instructions, a group's four matrix instructions cover them.
// (measured, cfg 2: with every lane drawing its eight calls ahead of the loop the counters cost 87 us of a 0.725 ms step)
struct BDrop { int train; unsigned spec; float scale; unsigned long long seed; unsigned step; int layer; };
struct KeepGen {
    uint4 c; unsigned k0, k1, own, give;
    unsigned long long call0; unsigned site, step, key0, key1, thr; int godd, train;
    // e_row: the row's first element (a multiple of 128: call-aligned)
    __device__ __forceinline__ void begin(const BDrop& d, int g, int kind, unsigned long long e_row) {
        const int gq = lane_id() >> 4;
        godd = gq & 1;
        call0 = (e_row >> 3) + (unsigned)(gq >> 1);            // call of column tile ct: call0 + 2 ct
        site = site_id(g, d.layer, kind); step = d.step; key0 = (unsigned)d.seed; key1 = (unsigned)(d.seed >> 32);
        thr = spec_thr(d.spec); train = d.train;
        own = 0u; give = 0u;
    }
    // slot s = 0 .. 63 of an MFMA loop (8 ct + j): call i = s / 16 in phases s % 16 = 0 (counter), 1 .. 10 (rounds), 11 (decisions)
    __device__ __forceinline__ void slot(int s) {
        const int i = s >> 4, ph = s & 15;
        const int ct = 2 * i + godd;
        if (ph == 0) {
            const unsigned long long call = call0 + 2u * (unsigned)ct;
            c = make_uint4((unsigned)call, (unsigned)(call >> 32), site, step);
            k0 = key0; k1 = key1;
        } else if (ph <= 10) {
#ifdef AMID_BS_ABLATE_PHILOX          // timing-only diagnostic build (profiles/tools/probe/bert_ablate.sh): what the rounds cost
            return;
#endif
            const unsigned long long p0 = mul_wide(0xD2511F53u, c.x), p1 = mul_wide(0xCD9E8D57u, c.z);
            c = make_uint4((unsigned)(p1 >> 32) ^ c.y ^ k0, (unsigned)p1, (unsigned)(p0 >> 32) ^ c.w ^ k1, (unsigned)p0);
            k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
        } else if (ph == 11) {
            const unsigned lo4 = ((c.x & 0xFFFFu) >= thr ? 1u : 0u) | ((c.x >> 16) >= thr ? 2u : 0u) | ((c.y & 0xFFFFu) >= thr ? 4u : 0u) | ((c.y >> 16) >= thr ? 8u : 0u);
            const unsigned hi4 = ((c.z & 0xFFFFu) >= thr ? 1u : 0u) | ((c.w >> 16) >= thr ? 8u : 0u) | ((c.z >> 16) >= thr ? 2u : 0u) | ((c.w & 0xFFFFu) >= thr ? 4u : 0u);
            own |= (godd ? hi4 : lo4) << (4 * ct);
            give |= (godd ? lo4 : hi4) << (4 * ct);
        }
    }
    __device__ __forceinline__ void hook(int ct, int j) { slot(ct * 8 + j); }
    // all four calls at once (no loop to hide them in)
    __device__ __forceinline__ void all() {
#pragma unroll
        for (int s = 0; s < 64; ++s) slot(s);
    }
    __device__ __forceinline__ unsigned finish() const {
        float a = __builtin_bit_cast(float, give), b = a;
        swap16(a, b);                                           // a: (r0, r0, r2, r2), b: (r1, r1, r3, r3) of `give` by lane row
        const unsigned got = __builtin_bit_cast(unsigned, godd ? a : b);
        return train ? (own | got) : ~0u;
    }
};
__device__ __forceinline__ unsigned keep_bits(const BDrop& d, int g, int kind, unsigned long long e_row) {
    KeepGen kg;
    kg.begin(d, g, kind, e_row);
    kg.all();
    return kg.finish();
}
__device__ __forceinline__ void apply_keep(StripRegs<BSD>& x, unsigned bits, float scale) {
#pragma unroll
    for (int ct = 0; ct < BNT; ++ct)
#pragma unroll
        for (int e = 0; e < 4; ++e) x.v[ct][e] = ((bits >> (4 * ct + e)) & 1u) ? x.v[ct][e] * scale : 0.f;
}

// a [2M, 512] tensor (pre, h, dpre): this lane's 16 bytes of column tile 0 of chunk 0; + 512 c + 64 ct for the others
__device__ __forceinline__ unsigned wide_off(const StripRow& row) {
    return row.ok ? row.off * 4u - 48u * (unsigned)(lane_id() >> 4) : STRIP_OOB;
}
__device__ __forceinline__ void wide_load(StripRegs<BSD>& x, const GBuf& g, unsigned offw, int c) {
#pragma unroll
    for (int ct = 0; ct < BNT; ++ct) x.v[ct] = g.load4(offw + c * (BSD * 4) + ct * 64);
}
// one column tile of chunk c per call, from inside an MFMA loop (first half of the loop, groups j == phase mod 4: as store_spread)
__device__ __forceinline__ void wide_spread(const GBuf& g, unsigned offw, int c, const StripRegs<BSD>& x, int ct, int j, int phase) {
    if (ct < BNT / 2 && (j & 3) == phase) { const int t = 2 * ct + (j >> 2); g.store4(offw + c * (BSD * 4) + t * 64, x.v[t]); }
}
__device__ __forceinline__ void spread_at(const GBuf& g, const StripRow& row, const StripRegs<BSD>& x, int ct, int j, int phase) {
    if (ct < BNT / 2 && (j & 3) == phase) strip_store_ct<BSD>(g, row, x, 2 * ct + (j >> 2));
}

// ================================================================================================================ forward
struct BStripQkvArgs {
    const float* x; const float* la[2]; const float* lb[2];
    const float* w[3][2]; const float* b[3][2];
    float* y; float* out[3];
};
struct BStripOffArgs {
    const float* o; const float* x;
    const float* wo[2]; const float* bo[2]; const float* la[2]; const float* lb[2];
    const float* w1[2]; const float* b1[2]; const float* w2[2]; const float* b2[2];
    float* x1; float* y2; float* pre; float* h; float* x2;
    const StepState* st; int train; unsigned spec; float scale; int layer;
};

// a saved tensor's buffer: a NULL pointer = "do not store" (a descriptor of 0 bytes: every store falls outside and is dropped)
__device__ __forceinline__ GBuf saved_buf(const float* p, unsigned bytes) { return GBuf(p, p != nullptr ? bytes : 0u); }

// q / k / v of one block on the strip X (in registers) -> Q, K, V (the callers that store them pass ONE strip as Q and V: q has left for
// global memory under k's matrix loop by the time v lands).  The ring's current fetch must be Wq of this block (started by the caller).
// XSTORE: X is also written to a.x (a fused predecessor produced it: the saved block input).
// SAVE = false (the inference kernel): nothing is stored -- no y, no q / k / v; the three strips are the result.
template <bool XSTORE, bool SAVE, class R>
__device__ __forceinline__ void bqkv_fwd_chain(const BStripQkvArgs& a, const StripGeom& sg, R& ring, const StripRow& row, int g,
                                               const StripRegs<BSD>& X, const ColVec<BSD>& la, const ColVec<BSD>& lb,
                                               StripRegs<BSD>& Q, StripRegs<BSD>& K, StripRegs<BSD>& V) {
    const GBuf gx = saved_buf(a.x, SAVE ? sg.act_bytes : 0u), gy = saved_buf(a.y, SAVE ? sg.act_bytes : 0u);
    StripRegs<BSD> Y;
    ColVec<BSD> bias;
    strip_lnb(Y, X, la, lb);
    f32x4 acc[BNT];
    {   // q = y Wq^T + bq ; x's and y's global copies leave under these MFMAs
        const float* buf = ring.next();
        bias.load(a.b[0][g]);
        strip_zero<BSD>(acc);
        strip_product<BSD, BSPREAD>(acc, Y, buf, ring, [&](int ct, int j) {
            ring.fetch(a.w[1][g], ct, j);
            if constexpr (XSTORE && SAVE) spread_at(gx, row, X, ct, j, 3);
            if constexpr (SAVE) spread_at(gy, row, Y, ct, j, 1);
        });
        add_bias<BSD>(acc, bias);
        to_regs<BSD>(Q, acc);
    }
    {   // k
        const float* buf = ring.next();
        bias.load(a.b[1][g]);
        strip_zero<BSD>(acc);
        const GBuf gq = saved_buf(a.out[0], SAVE ? sg.act_bytes : 0u);
        strip_product<BSD, BSPREAD>(acc, Y, buf, ring, [&](int ct, int j) {
            ring.fetch(a.w[2][g], ct, j);
            if constexpr (SAVE) spread_at(gq, row, Q, ct, j, 1);
        });
        add_bias<BSD>(acc, bias);
        to_regs<BSD>(K, acc);
    }
    {   // v
        const float* buf = ring.next();
        bias.load(a.b[2][g]);
        strip_zero<BSD>(acc);
        const GBuf gk = saved_buf(a.out[1], SAVE ? sg.act_bytes : 0u);
        strip_product<BSD, BSPREAD>(acc, Y, buf, ring, [&](int ct, int j) { if constexpr (SAVE) spread_at(gk, row, K, ct, j, 1); });
        add_bias<BSD>(acc, bias);
        to_regs<BSD>(V, acc);
        if constexpr (SAVE) strip_store<BSD>(saved_buf(a.out[2], sg.act_bytes), row, V);
    }
}

// out-projection + feed-forward of one block: A = the attention output o (in), X1 = the block input x (in) -> A = x2, the block output.
// The ring's current fetch must be Wo of this block.  NEXT: the last product fetches the next block's Wq (nx.w[0]) and the next block's
// LayerNorm vectors are requested into la / lb.  SAVE = false: x1, y2, pre, h are not stored.  DROP = false (inference): no dropout site
// draws its counters -- every keep bit is set; the multiplications by a.scale (1 outside training, a RUNTIME value) stay: without them the
// compiler forms other fused multiply-adds around the sites and the rows' low bits differ from the DROP build's (measured: ~2^-19).
template <bool NEXT, bool SAVE, bool DROP, class R>
__device__ __forceinline__ void boff_fwd_chain(const BStripOffArgs& a, const BStripQkvArgs& nx, const StripGeom& sg, R& ring, const StripRow& row,
                                               int g, StripRegs<BSD>& A, StripRegs<BSD>& X1, ColVec<BSD>& la, ColVec<BSD>& lb) {
    BDrop dc = {DROP ? a.train : 0, a.spec, a.scale, 0ull, 0u, a.layer};
    if (dc.train) { dc.seed = a.st->seed; dc.step = (unsigned)a.st->step; }
    const unsigned long long e128 = (unsigned long long)row.local * BSD, e512 = (unsigned long long)row.local * BSF;
    const unsigned wide_bytes = sg.act_bytes * 4u;
    const GBuf gx1 = saved_buf(a.x1, SAVE ? sg.act_bytes : 0u), gy2 = saved_buf(a.y2, SAVE ? sg.act_bytes : 0u),
               gpre = saved_buf(a.pre, SAVE ? wide_bytes : 0u), gh = saved_buf(a.h, SAVE ? wide_bytes : 0u);
    const unsigned offw = wide_off(row);
    StripRegs<BSD> Y2, P, Hc;
    ColVec<BSD> bias;
    bias.load(a.bo[g]); la.load(a.la[g]); lb.load(a.lb[g]);
    f32x4 acc[BNT], acc2[BNT];
    KeepGen kg;
    {   // x1 = x + drop_in(o Wo^T + bo) ; y2 = LNb_out(x1)
        if constexpr (DROP) kg.begin(dc, g, SITE_SUB_IN, e128);
        const float* buf = ring.next();
        strip_zero<BSD>(acc);
        strip_product<BSD, BSPREAD>(acc, A, buf, ring, [&](int ct, int j) { ring.fetch(a.w1[g], ct, j); if constexpr (DROP) kg.hook(ct, j); });
        add_bias<BSD>(acc, bias);
        to_regs<BSD>(A, acc);
        unsigned kb_in = ~0u;
        if constexpr (DROP) kb_in = kg.finish();
        apply_keep(A, kb_in, dc.scale);
#pragma unroll
        for (int ct = 0; ct < BNT; ++ct) X1.v[ct] += A.v[ct];
        strip_lnb(Y2, X1, la, lb);
    }
    strip_zero<BSD>(acc2);
    unsigned kb1 = ~0u, kb2 = ~0u;
    // (Tried, round 4: the eight products software-pipelined -- W1_0, W1_1, W2_0, W1_2, ... -- with chunk c's GELU + dropout inside the matrix
    // loop of the next product that does not need them, a column tile or an element per slot, forward and backward: the loops already carry
    // the dropout counters' rounds, the DMA pieces and the deferred stores, and the extra vector work stretches them by more than it saves
    // between them -- 0.6548 -> 0.6782 / 0.6657 ms per step; left as the plain chain.)
#pragma unroll
    for (int c = 0; c < BSC; ++c) {
        {   // pre_c = y2 W1_c^T + b1_c ; h_c = drop_ffn(gelu(pre_c))
            if constexpr (DROP) kg.begin(dc, g, SITE_FFN1, e512 + c * BSD);
            const float* buf = ring.next();
            bias.load(a.b1[g] + c * BSD);
            strip_zero<BSD>(acc);
            strip_product<BSD, BSPREAD>(acc, Y2, buf, ring, [&](int ct, int j) {
                bfetch_cols(ring, a.w2[g], c, ct, j);
                if constexpr (SAVE) if (c == 0) { spread_at(gx1, row, X1, ct, j, 1); spread_at(gy2, row, Y2, ct, j, 3); }
                if constexpr (DROP) kg.hook(ct, j);
            });
            unsigned kb = ~0u;
            if constexpr (DROP) kb = kg.finish();
            add_bias<BSD>(acc, bias);
            to_regs<BSD>(P, acc);
#pragma unroll
            for (int ct = 0; ct < BNT; ++ct)
#pragma unroll
#ifdef AMID_BS_ABLATE_GELU
                for (int e = 0; e < 4; ++e) Hc.v[ct][e] = P.v[ct][e] * 0.5f;
#else
                for (int e = 0; e < 4; ++e) Hc.v[ct][e] = gelu_f(P.v[ct][e]);
#endif
            apply_keep(Hc, kb, dc.scale);
        }
        {   // z += h_c W2_c^T ; pre_c's and h_c's global copies leave under these MFMAs (chunks 0 / 1: the decisions of the block's last two sites)
            if constexpr (DROP) {
                if (c == 0) kg.begin(dc, g, SITE_SUB_OUT, e128);
                if (c == 1) kg.begin(dc, g, SITE_BLOCK, e128);
            }
            const float* buf = ring.next();
            const float* nxt = c + 1 < BSC ? btile_rows<R>(a.w1[g], c + 1) : nx.w[0][g];
            strip_product<BSD, BSPREAD>(acc2, Hc, buf, ring, [&](int ct, int j) {
                if (NEXT || c + 1 < BSC) ring.fetch(nxt, ct, j);
                if constexpr (SAVE) {
                    wide_spread(gpre, offw, c, P, ct, j, 1);
                    wide_spread(gh, offw, c, Hc, ct, j, 3);
                }
                if constexpr (DROP) if (c < 2) kg.hook(ct, j);
            });
            if constexpr (DROP) {
                if (c == 0) kb1 = kg.finish();
                if (c == 1) kb2 = kg.finish();
            }
        }
    }
    {   // x2 = drop_block(x1 + drop_out(z + b2))
        bias.load(a.b2[g]);
        if constexpr (NEXT) { la.load(nx.la[g]); lb.load(nx.lb[g]); }
        add_bias<BSD>(acc2, bias);
        to_regs<BSD>(A, acc2);
        apply_keep(A, kb1, dc.scale);
#pragma unroll
        for (int ct = 0; ct < BNT; ++ct) A.v[ct] += X1.v[ct];
        apply_keep(A, kb2, dc.scale);
    }
}

}  // namespace amid
