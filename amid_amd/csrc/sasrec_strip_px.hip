// The backward strips of the SASRec layer, N-split build on producer-side bf16 pieces (round 6) -- the data gradients of sasrec_strip.hip's
// chains (strip_ffn_bwd_kernel, strip_qkv_bwd_kernel) with the forward's machinery (sasrec_seqn.hip seqn_fwd_px_body, seqn_parts.h):
// a workgroup = a 64-row tile = four 16-row strips x TWO column parts = eight waves, two per SIMD; a wave owns D / 2 output columns of every
// product, the operands made inside a chain cross the strip's two waves through LDS AS bf16 PIECES (xp_write: the next product's operand
// fragments), the transposed weights stream through three 32 KB plane slots (SeqRing3; the three-plane images of amid_step_head_w16_f32 /
// amid_embed_fwd_w16_f32).  Why: in the strip build a SIMD holds ONE wave, whose product is a chain of fragment reads and matrix
// instructions that nothing covers -- 6.5 us per 64 x 128 x 128 product against 1.3 us of matrix issue; the forward's build runs the same
// product in ~ 3 us with two waves per SIMD.  Reference: autograd of Log2feats.forward (model_seq.py:371-383) under loss.backward(),
// train_sr.py:214.  Same operations and operands as the strip build IN THE SAME ORDER -- a product walks its weight's mid / lo planes, then the
// hi plane, with the strip build's instruction order on every accumulator (PxbRing, pxb_mma_xp); a lane's row sums of the LayerNorm backward
// go on from its partner's column tile by column tile (pxb_row_chain) -- so the two builds give the SAME BITS: a training run does not
// depend on which build its steps took.  (With the forward's row statistics -- ln_stat, the _px_ entries -- the statistics are the forward's,
// added part by part there: agreement to rounding.)
#include "common.h"
#include "rng.h"
#include "strip_gemm.h"
#include "strip_chain.h"
#include "seq_fwd.h"
#include "seq_bwd.h"
#include "seqn_parts.h"
#include "sort_phases.h"
#include "scorer_sum.h"
#include "strip_px.h"

namespace amid {

constexpr int PXB_WPS = 4, PXB_NS = 2, PXB_NW = PXB_WPS * PXB_NS, PXB_THREADS = 64 * PXB_NW;
constexpr int PXB_STAT_STRIP = 2 * 64 + 2 * 16, PXB_STAT = PXB_WPS * PXB_STAT_STRIP;
// LDS: [three plane slots][four strips' exchange slots][row sums: strips x (2 x 64 lane sums + 2 x 16 row sums)][LayerNorm partials: strips x 2 x D]
// [the fused launch: the second chain's LayerNorm partials]
template <int D> constexpr size_t pxb_lds_floats(int chains = 1) {
    return (size_t)3 * (D * D / 2) + (size_t)PXB_WPS * XpStrip<D>::FLOATS + PXB_STAT + (size_t)chains * PXB_WPS * 2 * D;
}

// this lane's row of the tile: strip si, row m of it
struct PxbRow { unsigned off_own, phys; int local; bool ok; };
template <int D>
__device__ __forceinline__ PxbRow pxb_row(const StripGeom& sg, const StripTile& t, int si, int c0) {
    PxbRow r;
    int v = t.v0 + si * 16 + (lane_id() & 15);
    r.ok = v < t.nv;
    if (!r.ok) v = t.v0;
    if (sg.live != nullptr) {
        const int s = v / sg.T;
        r.local = sg.live[t.s0 + s] * sg.T + (v - s * sg.T);
    } else {
        r.local = v;
    }
    r.phys = (unsigned)t.g * (unsigned)sg.M + (unsigned)r.local;
    r.off_own = r.ok ? r.phys * (unsigned)(D * 4) + 16u * (unsigned)(lane_id() >> 4) + (unsigned)c0 * 64u : STRIP_OOB;
    return r;
}

// Two sums over the WHOLE row in the strip build's order: a lane of that build adds its elements column tile by column tile and the four
// lanes of a row then meet (row_sum4).  Here part 0's lane adds its tiles (`add(a, b)`: a, b += the own tiles' addends, in order), part 1's
// lane goes on from that lane's sums, meets its row and hands the row's sums back: the same additions in the same order, two barriers.
// (Calls may follow each other without a barrier between them: a slot is rewritten only behind the barrier its readers have passed.)
template <class Add>
__device__ __forceinline__ void pxb_row_chain(float* __restrict__ stat, int si, int part, float& a, float& b, const Add& add) {
    typedef __attribute__((address_space(3))) float lf;
    float* ls = stat + si * PXB_STAT_STRIP;
    float* rs = ls + 2 * 64;
    const int lane = lane_id(), m = lane & 15;
    a = 0.f; b = 0.f;
    if (part == 0) { add(a, b); lds_st1(ls + lane, a); lds_st1(ls + 64 + lane, b); }
    lds_barrier();
    if (part != 0) {
        a = *(lf*)(ls + lane); b = *(lf*)(ls + 64 + lane);
        add(a, b);
        a = row_sum4(a); b = row_sum4(b);
        if (lane < 16) { lds_st1(rs + m, a); lds_st1(rs + 16 + m, b); }
    }
    lds_barrier();
    if (part == 0) { a = *(lf*)(rs + m); b = *(lf*)(rs + 16 + m); }
}

// column sums over the strip's 16 rows of the own column tiles -> the strip's slice of the scratch [strips][2][D]
template <int D, int NCT>
__device__ __forceinline__ void pxb_ln_partials(float* __restrict__ scratch, int si, int c0, const PartRegs<NCT>& dgam, const PartRegs<NCT>& dbet) {
    const int lane = lane_id();
    float* mine = scratch + si * 2 * D;
#pragma unroll
    for (int c = 0; c < NCT; ++c) {
        f32x4 a, b;
#pragma unroll
        for (int r = 0; r < 4; ++r) { a[r] = col_sum16(dgam.v[c][r]); b[r] = col_sum16(dbet.v[c][r]); }
        if ((lane & 15) == 0) {
            lds_st4(mine + (c0 + c) * 16 + 4 * (lane >> 4), a);
            lds_st4(mine + D + (c0 + c) * 16 + 4 * (lane >> 4), b);
        }
    }
}
template <int D>
__device__ __forceinline__ void pxb_ln_partials_out(const float* __restrict__ scratch, float* __restrict__ part) {
    for (int e = threadIdx.x; e < 2 * D; e += PXB_THREADS)
        part[e] = (scratch[e] + scratch[2 * D + e]) + (scratch[4 * D + e] + scratch[6 * D + e]);
}

// LayerNorm backward of the strip over its column parts: DR = LN'(dy ; x, gamma) on the own columns, dy in `dbet` (the lane's addend of d beta),
// the lane's addends of d gamma left in `dgam`; the row's statistics given (have_stat: the forward's) or taken from x's row; every row sum
// in the strip build's order (strip_gemm.h strip_stats, sasrec_strip.hip strip_ln_bwd: the same bits).  Ends behind a workgroup barrier that
// every wave reaches after its last product.  addend: what is added to the result (the q / k / v chain's dk Wk + dv Wv) or nullptr.
// uout: receives u of DR = rstd u (rstd: the row's, returned) for xp_write_scaled.
template <int D, int NCT>
__device__ __forceinline__ void pxb_ln_bwd(PartRegs<NCT>& DR, const PartRegs<NCT>& dbet, const PartRegs<NCT>& X, const PartRegs<NCT>& gam, bool have_stat,
                                           float mean, float& rstd, float eps, float* __restrict__ stat, int si, int part, PartRegs<NCT>& dgam,
                                           const f32x4 (*addend)[NCT] = nullptr, PartRegs<NCT>* uout = nullptr) {
    if (!have_stat) {
        float tot, qt, dummy;
        pxb_row_chain(stat, si, part, tot, dummy, [&](float& s, float&) {
#pragma unroll
            for (int c = 0; c < NCT; ++c) s += (X.v[c][0] + X.v[c][1]) + (X.v[c][2] + X.v[c][3]);
        });
        mean = tot * (1.0f / D);
        pxb_row_chain(stat, si, part, qt, dummy, [&](float& q, float&) {
#pragma unroll
            for (int c = 0; c < NCT; ++c)
#pragma unroll
                for (int r = 0; r < 4; ++r) { const float d = X.v[c][r] - mean; q = fmaf(d, d, q); }
        });
        rstd = 1.0f / sqrtf(qt * (1.0f / D) + eps);
    }
    float t1, t2;
    pxb_row_chain(stat, si, part, t1, t2, [&](float& s1, float& s2) {
#pragma unroll
        for (int c = 0; c < NCT; ++c) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float dy = dbet.v[c][r];
                const float xh = (X.v[c][r] - mean) * rstd;
                float gy = gam.v[c][r] * dy;
                asm volatile("" : "+v"(gy));            // the rounded product (strip_ln_bwd)
                s1 += gy;
                s2 = fmaf(gy, xh, s2);
                float dg = dy * xh;
                asm volatile("" : "+v"(dg));
                dgam.v[c][r] = dg;
                DR.v[c][r] = gy;
            }
        }
    });
    const float c1 = t1 * (1.0f / D), c2 = t2 * (1.0f / D);
    {   // the strip build's instructions, spelled out (there the compiler contracts x - xh c2 and, where a sum follows, rstd u + addend into
        // fused multiply-adds; left to it here it chose otherwise for some elements: 1 ulp)
#pragma clang fp contract(off)
#pragma unroll
        for (int c = 0; c < NCT; ++c)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float xh = (X.v[c][r] - mean) * rstd;
                const float u = __builtin_fmaf(-xh, c2, DR.v[c][r] - c1);
                if (uout != nullptr) uout->v[c][r] = u;
                DR.v[c][r] = addend != nullptr ? __builtin_fmaf(rstd, u, (*addend)[c][r]) : rstd * u;
            }
    }
}

// xp_write of x = k u, elements rounded -- with the pieces the strip build makes of such a product: there the compiler contracts the
// multiplication into the split's first remainder, x - hi = fma(k, u, - hi): the remainder of the UNROUNDED product
template <int NCT>
__device__ __forceinline__ void xp_write_scaled(float* __restrict__ xps, int c0, const PartRegs<NCT>& u, float k) {
#pragma clang fp contract(off)
    const int lane = lane_id();
    auto split = [&](float ua, float ub) {
        WgSplit2 s;
        s.hi = wg_pack2(k * ua, k * ub);
        const float a1 = __builtin_fmaf(k, ua, -__uint_as_float(s.hi << 16)), b1 = __builtin_fmaf(k, ub, -__uint_as_float(s.hi & 0xffff0000u));
        s.mid = wg_pack2(a1, b1);
        const float a2 = a1 - __uint_as_float(s.mid << 16), b2 = b1 - __uint_as_float(s.mid & 0xffff0000u);
        s.lo = wg_pack2(a2, b2);
        return s;
    };
#pragma unroll
    for (int e = 0; e < NCT / 2; ++e) {
        const int st = c0 / 2 + e;
        const WgSplit2 p0 = split(u.v[2 * e][0], u.v[2 * e][1]), p1 = split(u.v[2 * e][2], u.v[2 * e][3]);
        const WgSplit2 p2 = split(u.v[2 * e + 1][0], u.v[2 * e + 1][1]), p3 = split(u.v[2 * e + 1][2], u.v[2 * e + 1][3]);
        lds_st4(xps + ((st * 3 + 0) * 64 + lane) * 4, __builtin_bit_cast(f32x4, amid_v4u{p0.hi, p1.hi, p2.hi, p3.hi}));
        lds_st4(xps + ((st * 3 + 1) * 64 + lane) * 4, __builtin_bit_cast(f32x4, amid_v4u{p0.mid, p1.mid, p2.mid, p3.mid}));
        lds_st4(xps + ((st * 3 + 2) * 64 + lane) * 4, __builtin_bit_cast(f32x4, amid_v4u{p0.lo, p1.lo, p2.lo, p3.lo}));
    }
}

// ---- a product in the strip build's order (strip_gemm.h strip_mma16x6): the weight's mid / lo planes against the operand's (mid, hi) pieces
// first, then the hi plane against (lo, mid, hi).  SeqRing3's three plane slots with the requests turned round: the NEXT weight's mid / lo
// planes are requested behind a product's first pass (M and L are free then: the hi pass, the epilogue and the next product's barrier ahead of
// their use), a product's hi plane when it begins (H is free then) and awaited behind its first pass.
template <int D, int NW> struct PxbRing : SeqRing3<D, NW> {
    using Base = SeqRing3<D, NW>;
    __device__ __forceinline__ explicit PxbRing(float* lds) : Base(lds) {}
    __device__ __forceinline__ void next() {               // everything requested so far has landed, every wave is past the previous product
        w_ring_wait();
        __syncthreads();
        if (!this->hi_ready) this->plane(this->hslot(), this->cur);
    }
    __device__ __forceinline__ void mid_sync() {           // behind the mid / lo pass: the hi plane has landed; M and L take the next weight's planes
        w_ring_wait();
        __syncthreads();
        this->plane(this->mslot(), this->nxt + (size_t)D * D);
        this->plane(this->lslot(), this->nxt + (size_t)2 * D * D);
        this->cur = this->nxt; this->hi_ready = false;
    }
};

// part_mma_xp (seqn_parts.h) with the passes in the strip build's order and its instruction order inside a step
template <int D, int NCT, class Ring>
__device__ __forceinline__ void pxb_mma_xp(f32x4 (&acc)[NCT], const float* __restrict__ xps, Ring& ring, int c0) {
    constexpr int KS = D / 32, NSTEP = KS * NCT, CT_BYTES = 16 * (D / 2) * 4, PLANE_BYTES = Ring::SLAB * 4;
    constexpr int PD1 = FRAG_AHEAD_2, PD2 = FRAG_AHEAD_1;
    static_assert(PD1 < NSTEP && PD2 < NSTEP && 2 * PD1 + 2 < 16, "read-ahead against the step count and the lgkmcnt field");
    const int lane = lane_id();
    const int i = lane & 15, g = lane >> 4;
    auto mma = [&](const f32x4& wf, const f32x4& a16, const f32x4& c) {
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(seqn_bf16x8, wf), __builtin_bit_cast(seqn_bf16x8, a16), c, 0, 0, 0);
    };
    unsigned fo[KS];                                          // this lane's fragment of k-step s in a plane, own column tile 0
#pragma unroll
    for (int s = 0; s < KS; ++s) fo[s] = (unsigned)((((c0 * 16 + i) * (D / 2)) + 4 * ((4 * s + g) ^ i)) * 4);
    const unsigned xa = lds_offset(xps) + (unsigned)lane * 16u;  // operand fragments: [k-step][piece][lane] x 16 bytes
    const unsigned mbase = lds_offset(ring.mslot());
    static_assert(CT_BYTES * (NCT - 1) + PLANE_BYTES < 65536, "the lo plane is reached through the offset field");
    const unsigned hbase = mbase + 2u * PLANE_BYTES;
    {   // first pass: mid x mid, lo x hi, mid x hi
        f32x4 wm[PD1 + 1], wl[PD1 + 1], ah[KS], am[KS];
        static_for<KS>([&](auto S) {
            constexpr int s = decltype(S)::value;
            lds_frag_issue<(s * 3 + 0) * 1024>(ah[s], xa);
            lds_frag_issue<(s * 3 + 1) * 1024>(am[s], xa);
        });
        auto issue = [&](auto U) {
            constexpr int u = decltype(U)::value, c = u / KS, s = u % KS, k = u % (PD1 + 1);
            lds_frag_issue<c * CT_BYTES>(wm[k], mbase + fo[s]);
            lds_frag_issue<c * CT_BYTES + PLANE_BYTES>(wl[k], mbase + fo[s]);
        };
        static_for<PD1>(issue);
        static_for<NSTEP>([&](auto T) {
            constexpr int t = decltype(T)::value, c = t / KS, s = t % KS, k = t % (PD1 + 1);
            if constexpr (t + PD1 < NSTEP) issue(std::integral_constant<int, t + PD1>{});
            constexpr int last = t + PD1 < NSTEP ? t + PD1 : NSTEP - 1;
            asm volatile("s_waitcnt lgkmcnt(%4)" : "+v"(wm[k]), "+v"(wl[k]), "+v"(ah[s]), "+v"(am[s]) : "n"(2 * (last - t)));
            acc[c] = mma(wm[k], am[s], acc[c]); acc[c] = mma(wl[k], ah[s], acc[c]); acc[c] = mma(wm[k], ah[s], acc[c]);
        });
    }
    ring.mid_sync();
    {   // second pass: the hi plane against the operand's three pieces
        f32x4 wf[PD2 + 1], ah[KS], am[KS], al[KS];
        static_for<KS>([&](auto S) {
            constexpr int s = decltype(S)::value;
            lds_frag_issue<(s * 3 + 0) * 1024>(ah[s], xa);
            lds_frag_issue<(s * 3 + 1) * 1024>(am[s], xa);
            lds_frag_issue<(s * 3 + 2) * 1024>(al[s], xa);
        });
        auto issue = [&](auto U) {
            constexpr int u = decltype(U)::value, c = u / KS, s = u % KS;
            lds_frag_issue<c * CT_BYTES>(wf[u % (PD2 + 1)], hbase + fo[s]);
        };
        static_for<PD2>(issue);
        static_for<NSTEP>([&](auto T) {
            constexpr int t = decltype(T)::value, c = t / KS, s = t % KS, k = t % (PD2 + 1);
            if constexpr (t + PD2 < NSTEP) issue(std::integral_constant<int, t + PD2>{});
            constexpr int last = t + PD2 < NSTEP ? t + PD2 : NSTEP - 1;
            asm volatile("s_waitcnt lgkmcnt(%4)" : "+v"(wf[k]), "+v"(ah[s]), "+v"(am[s]), "+v"(al[s]) : "n"(last - t));
            acc[c] = mma(wf[k], al[s], acc[c]); acc[c] = mma(wf[k], am[s], acc[c]); acc[c] = mma(wf[k], ah[s], acc[c]);
        });
    }
}

// one product of a chain: the next weight is announced, the deferred stores (an earlier product's result) leave in front of the matrix
// instructions (seqn_parts.h seqn_product_xp).  ZERO = false: the matrix instructions go on on what `acc` holds
template <int D, int NCT, bool ZERO = true, class Ring, class Stores>
__device__ __forceinline__ void pxb_product(f32x4 (&acc)[NCT], const float* __restrict__ xps, Ring& ring, const unsigned short* __restrict__ wn16, int c0,
                                            const Stores& stores) {
    if constexpr (ZERO) {
#pragma unroll
        for (int c = 0; c < NCT; ++c) acc[c] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    ring.begin(wn16);
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct) { stores(ct, 1); stores(ct, 3); }
    pxb_mma_xp<D, NCT, Ring>(acc, xps, ring, c0);
}

// the "== 0" bits of the own column tiles of the lane's row (tmq [2M, D / 4]: a byte per column quad)
template <int D, int NCT>
__device__ __forceinline__ void pxb_tm_load(unsigned (&bits)[NCT], const unsigned char* __restrict__ tmq, const StripGeom& sg, const PxbRow& row, int c0) {
    const GBuf gtm(tmq, sg.tm_bytes);
    const unsigned tbase = row.ok ? row.phys * (unsigned)(D / 4) + (unsigned)c0 * 4u : STRIP_OOB;
    const int sh = 8 * (lane_id() >> 4);
#pragma unroll
    for (int c = 0; c < NCT; ++c) bits[c] = (unsigned)__builtin_amdgcn_raw_buffer_load_b32(gtm.r, (int)(tbase + 4 * c), 0, 0) >> sh;
}
template <int NCT>
__device__ __forceinline__ void pxb_tm_apply(PartRegs<NCT>& x, const unsigned (&bits)[NCT]) {
#pragma unroll
    for (int c = 0; c < NCT; ++c) {
        x.v[c][0] = (bits[c] & 1u) ? 0.f : x.v[c][0];
        x.v[c][1] = (bits[c] & 2u) ? 0.f : x.v[c][1];
        x.v[c][2] = (bits[c] & 4u) ? 0.f : x.v[c][2];
        x.v[c][3] = (bits[c] & 8u) ? 0.f : x.v[c][3];
    }
}

// the loads the feed-forward backward needs first (relu output, "== 0" bits, LayerNorm gain, the forward's row statistics): issued by the
// caller ahead of the chain -- in front of the ring's first DMA pieces, or under a fused predecessor's last product
template <int NCT> struct PxbFfnPre { PartRegs<NCT> Hs, gam; unsigned tm[NCT]; float mean, rstd; };
template <int D, int NCT>
__device__ __forceinline__ void pxb_ffn_prefetch(PxbFfnPre<NCT>& p, const StripFfnBwdArgs& a, const float* __restrict__ ln_stat, const StripGeom& sg,
                                                 const PxbRow& row, int g, int c0) {
    part_load<NCT>(p.Hs, GBuf(a.h, sg.act_bytes), row.off_own);
    if (a.tmq != nullptr) pxb_tm_load<D, NCT>(p.tm, a.tmq, sg, row, c0);
    part_cols<NCT>(p.gam, a.ln_w[g], c0);
    p.mean = 0.f; p.rstd = 0.f;
    if (ln_stat != nullptr && row.ok) { p.mean = ln_stat[(long long)row.phys * 4 + 2]; p.rstd = ln_stat[(long long)row.phys * 4 + 3]; }
}

// d x' (own columns, in DZ) -> dpre2, dpre1, dr, d_o of the layer: strip_chain.h ffn_bwd_chain on the own column tiles.  The ring's pending
// weight must be w2T; `wnext`: the image the last product announces (any valid image: nothing follows the chain).
// ln_stat: the forward's row statistics [2M][4] (LN2's mean, rstd at +2) or nullptr (the statistics are taken from r's row then).
template <int D, int NCT, class Ring>
__device__ __forceinline__ void pxb_ffn_bwd_chain(const StripFfnBwdArgs& a, const float* __restrict__ ln_stat, const StripGeom& sg, Ring& ring,
                                                  const PxbRow& row, int g, int si, int part, int c0, PartRegs<NCT>& DZ, PxbFfnPre<NCT>& pre,
                                                  float* __restrict__ xps, float* __restrict__ stat, float* __restrict__ lnsc,
                                                  const unsigned short* __restrict__ wnext) {
    const GBuf gp2(a.dpre2, sg.act_bytes), gp1(a.dpre1, sg.act_bytes), gdr(a.dr, sg.act_bytes), gdo(a.d_o, sg.act_bytes);
    PartRegs<NCT> P, Rs;
    PartRegs<NCT>& Hs = pre.Hs;
    PartRegs<NCT>& gam = pre.gam;
    float mean = pre.mean, rstd = pre.rstd;
    if (a.tmq != nullptr) pxb_tm_apply<NCT>(DZ, pre.tm);
    // dpre2 = dz * drop2
    P = DZ;
    if (a.train) {
        const uint4 rr2 = rng_call(a.st->seed, (unsigned long long)row.local * D >> 7, site_id(g, a.layer, SITE_FFN2), (unsigned)a.st->step);
        part_dropout<NCT>(P, rr2, c0, a.spec, a.scale, (row.local * D) & 127);
    }
    xp_write<NCT>(xps, c0, P);
    f32x4 acc[NCT];
    {   // dh = dpre2 C2 ; dpre1 = dh * relu'(h) * drop1   (h > 0 implies the unit was kept by drop1)
        ring.next();
        part_load<NCT>(Rs, GBuf(a.r, sg.act_bytes), row.off_own);       // LN2 input rows: needed a product from now
        pxb_product<D, NCT>(acc, xps, ring, (const unsigned short*)a.w1T[g], c0, [&](int ct, int j) { part_spread<NCT>(gp2, row.off_own, P, ct, j, 1); });
#pragma unroll
        for (int c = 0; c < NCT; ++c)
#pragma unroll
            for (int r = 0; r < 4; ++r) P.v[c][r] = Hs.v[c][r] > 0.f ? acc[c][r] * a.scale : 0.f;
    }
    lds_barrier();                                      // the strip's two waves have read the last fragment of dpre2
    xp_write<NCT>(xps, c0, P);
    PartRegs<NCT> DR, U, dgam, dbet;
    {   // dy = dpre1 C1 + dz ; dr = LN2'(dy ; r)
        ring.next();
        pxb_product<D, NCT>(acc, xps, ring, (const unsigned short*)a.woT[g], c0, [&](int ct, int j) { part_spread<NCT>(gp1, row.off_own, P, ct, j, 1); });
#pragma unroll
        for (int c = 0; c < NCT; ++c) dbet.v[c] = acc[c] + DZ.v[c];
        pxb_ln_bwd<D, NCT>(DR, dbet, Rs, gam, ln_stat != nullptr, mean, rstd, a.ln_eps, stat, si, part, dgam, nullptr, &U);
        pxb_ln_partials<D, NCT>(lnsc, si, c0, dgam, dbet);
    }
    // (the row sums' barrier lies behind the last fragment read of dpre1: the slots are free)
    xp_write_scaled<NCT>(xps, c0, U, rstd);
    {   // d_o = dr Wo
        ring.next();
        pxb_product<D, NCT>(acc, xps, ring, wnext, c0, [&](int ct, int j) { part_spread<NCT>(gdr, row.off_own, DR, ct, j, 1); });
#pragma unroll
        for (int c = 0; c < NCT; ++c) P.v[c] = acc[c];
        part_store<NCT>(gdo, row.off_own, P);
    }
}

// dq, dk, dv, dr of a layer -> d x (own columns, left in DX): strip_chain.h's qkv_bwd_chain on the wave's own column tiles.  The ring's pending
// weight must be wkT; Dk, Dv: the own columns of dk, dv (the caller requested them in front of the ring's first pieces); `wnext`: the image
// the last product announces (a fused successor's first weight, or any valid image); `before_last()` runs in front of the last product (a
// fused successor issues its first loads there).  ln_stat: the forward's row statistics [2M][4] (LN1's mean, rstd at +0) or nullptr.
template <int D, int NCT, class Ring, class Hook>
__device__ __forceinline__ void pxb_qkv_bwd_chain(const StripQkvBwdArgs& a, const float* __restrict__ ln_stat, const StripGeom& sg, Ring& ring,
                                                  const PxbRow& row, int g, int si, int part, int c0, const PartRegs<NCT>& Dk, const PartRegs<NCT>& Dv,
                                                  PartRegs<NCT>& DX, float* __restrict__ xps, float* __restrict__ stat, float* __restrict__ lnsc,
                                                  const unsigned short* __restrict__ wnext, const Hook& before_last) {
    PartRegs<NCT> Dq, Drs, Xs, gam;
    f32x4 acc_kv[NCT], acc[NCT];
    const auto none = [](int, int) {};
    xp_write<NCT>(xps, c0, Dk);
    {   // dk Wk          (every operand is requested a product ahead of its use)
        ring.next();
        part_load<NCT>(Dq, GBuf(a.dq, sg.act_bytes), row.off_own);
        pxb_product<D, NCT>(acc_kv, xps, ring, (const unsigned short*)a.wvT[g], c0, none);
    }
    lds_barrier();                                      // the strip's two waves have read the last fragment of dk
    xp_write<NCT>(xps, c0, Dv);
    float mean = 0.f, rstd = 0.f;
    {   // + dv Wv        (the matrix instructions go on on the same accumulators)
        ring.next();
        part_load<NCT>(Drs, GBuf(a.dr, sg.act_bytes), row.off_own);     // residual-path gradient of the normed query
        part_load<NCT>(Xs, GBuf(a.x, sg.act_bytes), row.off_own);       // LN1 input rows
        part_cols<NCT>(gam, a.ln_w[g], c0);
        if (ln_stat != nullptr && row.ok) { mean = ln_stat[(long long)row.phys * 4]; rstd = ln_stat[(long long)row.phys * 4 + 1]; }
        pxb_product<D, NCT, false>(acc_kv, xps, ring, (const unsigned short*)a.wqT[g], c0, none);
    }
    lds_barrier();
    xp_write<NCT>(xps, c0, Dq);
    PartRegs<NCT> dgam;
    {   // dqn = dq Wq + dr ; dx = LN1'(dqn ; x) + (dk Wk + dv Wv)
        ring.next();
        before_last();
        pxb_product<D, NCT>(acc, xps, ring, wnext, c0, none);
#pragma unroll
        for (int c = 0; c < NCT; ++c) Drs.v[c] += acc[c];
        pxb_ln_bwd<D, NCT>(DX, Drs, Xs, gam, ln_stat != nullptr, mean, rstd, a.ln_eps, stat, si, part, dgam, &acc_kv);
    }
    pxb_ln_partials<D, NCT>(lnsc, si, c0, dgam, Drs);
}

// the waves of a tile: strip si of four, column part `part` of two, own column tiles [c0, c0 + NCT)
struct PxbWave { int part, si, c0; };
template <int NCT> __device__ __forceinline__ PxbWave pxb_wave() {
    const int w = wave_id();
    return PxbWave{w / PXB_WPS, w % PXB_WPS, (w / PXB_WPS) * NCT};
}
template <int D> __device__ __forceinline__ float* pxb_xps(float* smem, int si) { return smem + 3 * SeqRing3<D, PXB_NW>::SLAB + si * XpStrip<D>::FLOATS; }
template <int D> __device__ __forceinline__ float* pxb_stat(float* smem) { return smem + 3 * SeqRing3<D, PXB_NW>::SLAB + PXB_WPS * XpStrip<D>::FLOATS; }
template <int D> __device__ __forceinline__ float* pxb_lnsc(float* smem, int which) { return pxb_stat<D>(smem) + PXB_STAT + which * PXB_WPS * 2 * D; }

// RIDER: 0, or the phase of the step's index sort the first rd.plan.nblk workgroups run (their first four waves; sort_phases.h)
// The tile's first operand loads are issued IN FRONT of the ring's first DMA pieces (behind them they waited out the pieces' issue: the
// stamps put ~ 8 k cycles in front of the first product); a dead tile then leaves without having started a DMA.
template <int D, int RIDER>
__global__ __launch_bounds__(PXB_THREADS) void strip_ffn_bwd_px_kernel(const StripFfnBwdArgs a, const float* __restrict__ ln_stat, const StripGeom sg,
                                                                       const SortRider rd) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int NCT = D / 16 / PXB_NS;
    int bid = blockIdx.x;
    if constexpr (RIDER != 0) {
        if (bid < rd.plan.nblk) { if (threadIdx.x < SORT_THREADS) sort_phase_ct<RIDER>(rd.plan, bid, smem); return; }
        bid -= rd.plan.nblk;
    }
    const PxbWave wv = pxb_wave<NCT>();
    const StripTile t = strip_tile(sg, bid);
    if (!t.live) { zero_slot<D>(a.ln_part, t.slot); return; }
    const int g = t.g;
    const PxbRow row = pxb_row<D>(sg, t, wv.si, wv.c0);
    PartRegs<NCT> DZ;
    PxbFfnPre<NCT> pre;
    part_load<NCT>(DZ, GBuf(a.dxo, sg.act_bytes), row.off_own);
    pxb_ffn_prefetch<D, NCT>(pre, a, ln_stat, sg, row, g, wv.c0);
    PxbRing<D, PXB_NW> ring(smem);
    ring.first((const unsigned short*)a.w2T[g]);
    float* const lnsc = pxb_lnsc<D>(smem, 0);
    pxb_ffn_bwd_chain<D, NCT>(a, ln_stat, sg, ring, row, g, wv.si, wv.part, wv.c0, DZ, pre, pxb_xps<D>(smem, wv.si), pxb_stat<D>(smem), lnsc,
                              (const unsigned short*)a.woT[g]);
    w_ring_wait();                                      // (the last product announced a plane: its DMA must not outlive the workgroup's LDS)
    __syncthreads();
    pxb_ln_partials_out<D>(lnsc, a.ln_part + (long long)t.slot * 2 * D);
}

// strip_qkv_bwd_kernel (sasrec_strip.hip) in the N-split form.  FFN = true: the layer below's feed-forward / out-projection backward goes on
// on d x, which stays in registers and crosses to the strip's partner wave as pieces (never stored); FFN = false: d x is stored, with the
// embedding layer's backward applied on the own columns when a.emb_tmq is set.  RIDER: as strip_qkv_bwd_kernel -- with FFN phase 3, without
// phase 4 of the sort as the first rd.plan.nblk workgroups; != 0 with FFN: the scorer sums' workgroups behind the tiles or (ss.front) in front
// of everything; -1: those without a sort rider.  A rider workgroup runs on the first four waves, its LDS the head of the allocation.
template <int D, bool FFN, int RIDER>
__global__ __launch_bounds__(PXB_THREADS) void strip_qkv_bwd_px_kernel(const StripQkvBwdArgs a, const StripFfnBwdArgs f, const float* __restrict__ ln_stat,
                                                                       const float* __restrict__ f_ln_stat, const ScorerSum ss, const StripGeom sg,
                                                                       const SortRider rd) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int NCT = D / 16 / PXB_NS;
    int bid = blockIdx.x;
    if constexpr (RIDER != 0 && FFN) {
        if (ss.front) {
            if (bid < ss.nblk) { if (threadIdx.x < STRIP_THREADS) scorer_sum_block(ss, bid, (scorer_lds_f4*)smem); return; }
            bid -= ss.nblk;
        } else {
            const int first = (int)gridDim.x - ss.nblk;
            if (bid >= first) { if (threadIdx.x < STRIP_THREADS) scorer_sum_block(ss, bid - first, (scorer_lds_f4*)smem); return; }
        }
    }
    if constexpr (RIDER > 0) {
        if (bid < rd.plan.nblk) { if (threadIdx.x < SORT_THREADS) sort_phase_ct<RIDER>(rd.plan, bid, smem); return; }
        bid -= rd.plan.nblk;
    }
    const PxbWave wv = pxb_wave<NCT>();
    const StripTile t = strip_tile(sg, bid);
    if (!t.live) {
        zero_slot<D>(a.ln_part, t.slot);
        if constexpr (FFN) zero_slot<D>(f.ln_part, t.slot);
        return;
    }
    const int g = t.g;
    const PxbRow row = pxb_row<D>(sg, t, wv.si, wv.c0);
    PartRegs<NCT> Dk, Dv, DX;
    part_load<NCT>(Dk, GBuf(a.dk, sg.act_bytes), row.off_own);
    part_load<NCT>(Dv, GBuf(a.dv, sg.act_bytes), row.off_own);
    PxbRing<D, PXB_NW> ring(smem);
    ring.first((const unsigned short*)a.wkT[g]);
    float* const xps = pxb_xps<D>(smem, wv.si);
    float* const stat = pxb_stat<D>(smem);
    if constexpr (FFN) {
        PxbFfnPre<NCT> pre;
        pxb_qkv_bwd_chain<D, NCT>(a, ln_stat, sg, ring, row, g, wv.si, wv.part, wv.c0, Dk, Dv, DX, xps, stat, pxb_lnsc<D>(smem, 0),
                                  (const unsigned short*)f.w2T[g], [&]() { pxb_ffn_prefetch<D, NCT>(pre, f, f_ln_stat, sg, row, g, wv.c0); });
        pxb_ffn_bwd_chain<D, NCT>(f, f_ln_stat, sg, ring, row, g, wv.si, wv.part, wv.c0, DX, pre, xps, stat, pxb_lnsc<D>(smem, 1),
                                  (const unsigned short*)f.woT[g]);
    } else {
        const bool emb = a.emb_tmq != nullptr;                 // (uniform) the embedding layer's backward on the strip: see StripQkvBwdArgs
        unsigned etm[NCT];
        pxb_qkv_bwd_chain<D, NCT>(a, ln_stat, sg, ring, row, g, wv.si, wv.part, wv.c0, Dk, Dv, DX, xps, stat, pxb_lnsc<D>(smem, 0),
                                  (const unsigned short*)a.wkT[g], [&]() { if (emb) pxb_tm_load<D, NCT>(etm, a.emb_tmq, sg, row, wv.c0); });
        if (emb) {
            if (a.emb_train) {
                const uint4 rr = rng_call(a.emb_st->seed, (unsigned long long)row.local * D >> 7, site_id(g, 0, SITE_EMB), (unsigned)a.emb_st->step);
                part_dropout<NCT>(DX, rr, wv.c0, a.emb_spec, a.emb_scale, (row.local * D) & 127);
            }
            pxb_tm_apply<NCT>(DX, etm);
        }
        part_store<NCT>(GBuf(a.dx, sg.act_bytes), row.off_own, DX);
    }
    w_ring_wait();                                      // (the last product announced a plane: its DMA must not outlive the workgroup's LDS)
    __syncthreads();
    pxb_ln_partials_out<D>(pxb_lnsc<D>(smem, 0), a.ln_part + (long long)t.slot * 2 * D);
    if constexpr (FFN) pxb_ln_partials_out<D>(pxb_lnsc<D>(smem, 1), f.ln_part + (long long)t.slot * 2 * D);
}

// ---- host side: the launches of the N-split builds (strip_px.h) ----
using namespace amid_strip_host;

// part_dropout draws a row's keep bits from ONE Philox call: p = 0.5 (or no dropout)
static bool pxb_dropout_ok(int train, unsigned spec) { return !train || spec_bits(spec) == 1; }

int launch_ffn_bwd_px(const StripFfnBwdArgs& a, const float* ln_stat, const StripGeom& sg, const SortRider& rd, void* stream) {
    if (!pxb_dropout_ok(a.train, a.spec)) return AMID_ERR_UNSUPPORTED;
    if (rd.phase != 0 && rd.phase != 2) return AMID_ERR_UNSUPPORTED;           // this launch carries phase 2
    constexpr size_t lds = pxb_lds_floats<128>() * sizeof(float);
    static_assert(lds >= sizeof(SortScatterLds<OS_BINS_MAX>), "the rider's scatter fits the head of the allocation");
    if (rd.phase != 0) return launch_lds<strip_ffn_bwd_px_kernel<128, 2>>(2 * sg.tpg + rd.plan.nblk, PXB_THREADS, lds, stream, a, ln_stat, sg, rd);
    return launch_lds<strip_ffn_bwd_px_kernel<128, 0>>(2 * sg.tpg, PXB_THREADS, lds, stream, a, ln_stat, sg, rd);
}

int launch_qkv_bwd_px(const StripQkvBwdArgs& a, const StripFfnBwdArgs& f, bool ffn, const float* ln_stat, const float* f_ln_stat, const ScorerSum& ss,
                      const StripGeom& sg, const SortRider& rd, void* stream) {
    if (!pxb_dropout_ok(a.emb_train, a.emb_spec) || (ffn && !pxb_dropout_ok(f.train, f.spec))) return AMID_ERR_UNSUPPORTED;
    if (rd.phase != 0 && rd.phase != (ffn ? 3 : 4)) return AMID_ERR_UNSUPPORTED;
    if (ss.nblk > 0 && !ffn) return AMID_ERR_UNSUPPORTED;                      // the scorer sums ride on the fused launch
    constexpr size_t lds1 = pxb_lds_floats<128>(1) * sizeof(float), lds2 = pxb_lds_floats<128>(2) * sizeof(float);
    static_assert(lds2 <= 160 * 1024, "the fused launch's second LayerNorm scratch fits the CU's LDS");
    static_assert(lds1 >= sizeof(SortScatterLds<OS_BINS_MAX>) && lds1 >= 8 * 33 * 16, "a rider's scratch fits the head of the allocation");
    const int tiles = 2 * sg.tpg, sortb = rider_blocks_host(rd);
    if (ffn) {
        if (rd.phase) return launch_lds<strip_qkv_bwd_px_kernel<128, true, 3>>(tiles + sortb + ss.nblk, PXB_THREADS, lds2, stream, a, f, ln_stat, f_ln_stat, ss, sg, rd);
        // (without a sort rider: one build, with or without the scorer sums' workgroups -- ss.nblk = 0: none of its workgroups is one)
        return launch_lds<strip_qkv_bwd_px_kernel<128, true, -1>>(tiles + ss.nblk, PXB_THREADS, lds2, stream, a, f, ln_stat, f_ln_stat, ss, sg, rd);
    }
    if (rd.phase) return launch_lds<strip_qkv_bwd_px_kernel<128, false, 4>>(tiles + sortb, PXB_THREADS, lds1, stream, a, f, ln_stat, f_ln_stat, ss, sg, rd);
    return launch_lds<strip_qkv_bwd_px_kernel<128, false, 0>>(tiles, PXB_THREADS, lds1, stream, a, f, ln_stat, f_ln_stat, ss, sg, rd);
}

}  // namespace amid

using namespace amid;
using namespace amid_strip_host;

// amid_sas_strip_ffn_bwd_f32 (mma_bf16 = 3: the weights are three-plane images of the transposes) as the N-split build on pieces.
// ln_stat: the forward's row statistics of this layer ([2 B T][4]: LN2's mean and rstd at +2) or NULL.  sort_plan / sort_phase: optional rider.
extern "C" int amid_sas_strip_ffn_bwd_px_f32(const float* dxo, const unsigned char* tmq, const float* h, const float* r, const float* const* ln_w,
                                             const float* const* w1T, const float* const* w2T, const float* const* woT, float ln_eps, int B, int T,
                                             int D, const int* live, int layer, const void* step_state, int train, float p_drop, float* dpre2,
                                             float* dpre1, float* dr, float* d_o, float* ln_part, const float* ln_stat, const void* sort_plan,
                                             int sort_phase, void* stream) {
    AMID_FFN_BWD_CALL(c);
    AMID_CHECK_ARG(c.dxo && c.operands());
    if (D != 128) return AMID_ERR_UNSUPPORTED;
    if (train && p_drop > 0.f && spec_bits(drop_spec(p_drop)) != 1) return AMID_ERR_UNSUPPORTED;       // part_dropout: p = 0.5
    StripGeom sg;
    if (int e = make_strip_geom(B, T, D, live, &sg)) return e;
    StripFfnBwdArgs a;
    fill_ffn_bwd(a, c);
    SortRider rd;
    rd.phase = 0;
    if (sort_plan != nullptr) {
        if (sort_phase != 2) return AMID_ERR_UNSUPPORTED;
        rd.plan = *(const SortPlan*)sort_plan;
        rd.phase = sort_phase;
    }
    return launch_ffn_bwd_px(a, ln_stat, sg, rd, stream);
}
#undef AMID_FFN_BWD_CALL
