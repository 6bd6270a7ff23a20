// BERT4Rec encoder block as register-resident strip chains (strip_gemm.h / strip_chain.h), forward and backward.
// Reference arithmetic: TransformerBlock.forward model_seq.py:242-245 with SublayerConnection :140-142, the hand-written LayerNorm
// :124-127 (UNBIASED std, eps added to the std), MultiHeadedAttention's projections :183-196, PositionwiseFeedForward :216-217 with the
// tanh GELU :204 -- hidden 128 / 4 heads / feed-forward 512 / dropout 0.1 hard-coded by the reference (:264-267) -- and their autograd
// (loss.backward(), train_sr.py:214).  Same operations, operands, dropout counters and saved tensors as the row-tile kernels of bert.hip
// (which stay for activations beyond 2 GiB); the attention core between the projections runs in its own launch
// (attention_mfma_bert.hip).
//
//   bert_strip_qkv_fwd        y = LNb_in(x) ; q, k, v = y W{0,1,2}^T + b                                     (all three from the normed y)
//   bert_strip_oproj_ffn_fwd  x1 = x + drop_in(o Wo^T + bo) ; y2 = LNb_out(x1) ; per 128-column chunk c of the 512 hidden units:
//                             pre_c = y2 W1_c^T + b1_c, h_c = drop_ffn(gelu(pre_c)), z += h_c W2_c^T ;
//                             x2 = drop_block(x1 + drop_out(z + b2))        [+ the next block's bert_strip_qkv_fwd on x2 in registers]
//   bert_strip_ffn_bwd        dr = dx2 * drop_block ; dz = dr * drop_out ; per chunk: dpre_c = (dz W2_c) * drop_ffn * gelu'(pre_c),
//                             dy2 += dpre_c W1_c ; dx1 = LNb_out'(dy2 ; x1) + dr ; dt = dx1 * drop_in ; d_o = dt Wo
//   bert_strip_qkv_bwd        dx = LNb_in'(dq Wq + dk Wk + dv Wv ; x) + dx1      [+ the block below's bert_strip_ffn_bwd on dx in registers]
// A wave owns 16 rows and all 128 columns; a workgroup is 4 waves = 64 rows of one domain; in a train step only the LIVE sequences
// are walked (StripGeom::live).  The 128 x 128 weight tiles stream through the two-slab LDS ring by LDS-DMA; the tiles of w_2
// [128, 512] and of the transposed w_1 [128, 512] are column blocks of a 512-float row (WDmaLd).  Backward weights arrive TRANSPOSED
// (amid_transpose_rect_f32) so that a data gradient is again C[rows, N] = A[rows, K] W'[N, K]^T.  2 D D FLOP per row and tile.
#include "common.h"
#include "rng.h"
#include "strip_gemm.h"
#include "strip_chain.h"
#include "bert_math.h"
#include "weights_image.h"
#include "bert_strip_parts.h"

namespace amid {


// Riders of the step's FIRST strip launch (workgroups behind the tiles'; the live tiles of a train step leave a fifth of the CUs free):
// the key mask of both encoders (model_seq.py:288: seq_d2 > 0) for the attention launch that follows, and the transposed weights the
// backward's data gradients multiply with -- two launches of their own until now (amid_key_keep_u8, amid_transpose_rect_f32).
constexpr int BPRO_MAX = 24;
struct BPrologue {
    const long long* seq; unsigned char* keep; int n_keys;       // keep[i] = seq[i] > 0; seq == nullptr: none
    const float* src[BPRO_MAX]; float* dst[BPRO_MAX]; int rows[BPRO_MAX], cols[BPRO_MAX]; int n;      // dst[c][r] = src[r][c]; rows, cols multiples of 64
    int blocks;
};
__device__ __forceinline__ void bert_prologue_block(const BPrologue& p, int blk, float* __restrict__ lds) {
    if (p.seq != nullptr)
        for (int i = blk * STRIP_THREADS + threadIdx.x; i < p.n_keys; i += p.blocks * STRIP_THREADS) p.keep[i] = p.seq[i] > 0 ? 1 : 0;
    float (*tile)[65] = (float (*)[65])lds;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    int unit0 = 0;                                               // 64 x 64 units of all matrices, dealt round-robin over the rider blocks
    for (int m = 0; m < p.n; ++m) {
        const int R = p.rows[m], C = p.cols[m];
        const int tilesx = C / 64, tiles = tilesx * (R / 64);
        const int first = (blk - unit0 % p.blocks + p.blocks) % p.blocks;
        for (int tt = first; tt < tiles; tt += p.blocks) {
            const int bx = (tt % tilesx) * 64, by = (tt / tilesx) * 64;
            __syncthreads();
            float v[16];
#pragma unroll
            for (int k = 0; k < 8; ++k) {                          // sixteen loads in flight per thread
                const float* sp = p.src[m] + (long long)(by + ty + 8 * k) * C + bx + tx;
                v[2 * k] = sp[0]; v[2 * k + 1] = sp[32];
            }
#pragma unroll
            for (int k = 0; k < 8; ++k) { tile[ty + 8 * k][tx] = v[2 * k]; tile[ty + 8 * k][tx + 32] = v[2 * k + 1]; }
            __syncthreads();
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                float* dp = p.dst[m] + (long long)(bx + ty + 8 * k) * R + by + tx;
                dp[0] = tile[tx][ty + 8 * k]; dp[32] = tile[tx + 32][ty + 8 * k];
            }
        }
        unit0 += tiles;
    }
}

template <int MODE>
__global__ __launch_bounds__(STRIP_THREADS) void bert_strip_qkv_fwd_kernel(const BStripQkvArgs a, const StripGeom sg, const BPrologue pro) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    if ((int)blockIdx.x >= 2 * sg.tpg) { bert_prologue_block(pro, blockIdx.x - 2 * sg.tpg, smem); return; }
    typename BRingSel<MODE>::type ring(smem);
    ring.first(a.w[0][strip_domain(blockIdx.x)]);
    const StripTile t = strip_tile(sg, blockIdx.x);
    if (!t.live) { w_ring_wait(); return; }
    const StripRow row = strip_row<BSD>(sg, t);
    StripRegs<BSD> X;
    ColVec<BSD> la, lb;
    strip_load<BSD>(X, GBuf(a.x, sg.act_bytes), row);
    la.load(a.la[t.g]); lb.load(a.lb[t.g]);
    StripRegs<BSD> P0, P1;
    bqkv_fwd_chain<false, true>(a, sg, ring, row, t.g, X, la, lb, P0, P1, P0);
}

template <bool NEXT, int MODE>
__global__ __launch_bounds__(STRIP_THREADS) void bert_strip_oproj_ffn_fwd_kernel(const BStripOffArgs a, const BStripQkvArgs nx, const StripGeom sg) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    using R = typename BRingSel<MODE>::type;
    R ring(smem);
    ring.first(a.wo[strip_domain(blockIdx.x)]);
    const StripTile t = strip_tile(sg, blockIdx.x);
    if (!t.live) { w_ring_wait(); return; }
    const StripRow row = strip_row<BSD>(sg, t);
    const int g = t.g;
    StripRegs<BSD> A, X1;
    ColVec<BSD> la, lb;
    strip_load<BSD>(A, GBuf(a.o, sg.act_bytes), row);
    strip_load<BSD>(X1, GBuf(a.x, sg.act_bytes), row);
    boff_fwd_chain<NEXT, true, true>(a, nx, sg, ring, row, g, A, X1, la, lb);
    if constexpr (NEXT) {
        StripRegs<BSD> P0, P1;
        bqkv_fwd_chain<true, true>(nx, sg, ring, row, g, A, la, lb, P0, P1, P0);
    } else {
        strip_store<BSD>(GBuf(a.x2, sg.act_bytes), row, A);
    }
}

// ================================================================================================================ backward
struct BStripFfnBwdArgs {
    const float* dx2; const float* pre; const float* x1; const float* la[2];           // LNb_out gamma
    const float* w2T[2]; const float* w1T[2]; const float* woT[2];                   // [512,128] ; [128,512] ; [128,128]
    float* dz; float* dpre; float* dx1; float* dt; float* d_o; float* ln_part;      // [2M,128], [2M,512], [2M,128] x 3, [2 tpg][2][128]
    const StepState* st; int train; unsigned spec; float scale; int layer;
};
struct BStripQkvBwdArgs {
    const float* dq; const float* dk; const float* dv; const float* dx1; const float* x; const float* la[2];     // LNb_in gamma
    const float* wT[3][2];
    float* dx; float* ln_part;
    int zero_blocks;        // > 0 (live list given, dx written): that many extra workgroups behind the tiles' zero the rows of dx the live walk
                            // never writes -- the DEAD sequences' (their gradient is exactly zero; the segment reduce reads every row)
};

// dead sequence j of the live list: the other domain's sequence of the sample live[j]
__device__ __forceinline__ void zero_dead_rows(float* __restrict__ dx, const StripGeom& sg, int blk, int nblk) {
    const int n0 = sg.live[sg.B];
    const int q = sg.T * (BSD / 4);
    for (int j = blk; j < sg.B; j += nblk) {
        const int g_dead = j < n0 ? 1 : 0;
        float* base = dx + ((long long)g_dead * sg.M + (long long)sg.live[j] * sg.T) * BSD;
        for (int i = threadIdx.x; i < q; i += STRIP_THREADS) st4_global(base + 4 * i, make_float4(0.f, 0.f, 0.f, 0.f));
    }
}

// d x2 (DX2, in registers) -> dz, dpre, dx1, dt, d_o of this block; the ring's current fetch must be chunk 0 of w2T.
// TAIL: a slab (`tail`) is fetched under the last MFMA loop (a fused successor's first weight).
// kb_block / kb_out: the keep bits of the block's last two dropout sites (bffn_drop(a) + keep_bits, or drawn by a fused predecessor
// under its own matrix loops)
__device__ __forceinline__ BDrop bffn_drop(const BStripFfnBwdArgs& a) {
    BDrop dc = {a.train, a.spec, a.scale, 0ull, 0u, a.layer};
    if (a.train) { dc.seed = a.st->seed; dc.step = (unsigned)a.st->step; }
    return dc;
}
template <class R>
__device__ __forceinline__ void bffn_bwd_chain(const BStripFfnBwdArgs& a, const StripGeom& sg, R& ring, const StripRow& row, int g,
                                               StripRegs<BSD>& DX2, float* __restrict__ scratch, unsigned kb_block, unsigned kb_out) {
    const BDrop dc = bffn_drop(a);
    const unsigned long long e128 = (unsigned long long)row.local * BSD, e512 = (unsigned long long)row.local * BSF;
    const unsigned wide_bytes = sg.act_bytes * 4u;
    const GBuf gpre(a.pre, wide_bytes), gdpre(a.dpre, wide_bytes), gdz(a.dz, sg.act_bytes), gdx1(a.dx1, sg.act_bytes), gdt(a.dt, sg.act_bytes);
    const unsigned offw = wide_off(row);
    StripRegs<BSD> DZ, DP, PRE, X1;
    ColVec<BSD> gam;
    // dr = dx2 * drop_block (kept in DX2: the residual path into x1) ; dz = dr * drop_out
    apply_keep(DX2, kb_block, dc.scale);
    DZ = DX2;
    apply_keep(DZ, kb_out, dc.scale);
    KeepGen kg;
    unsigned kb_in = ~0u;
    f32x4 acc[BNT], accy[BNT];
    strip_zero<BSD>(accy);
#pragma unroll
    for (int c = 0; c < BSC; ++c) {
        {   // dh_c = dz W2_c ; dpre_c = dh_c * drop_ffn * gelu'(pre_c)
            kg.begin(dc, g, SITE_FFN1, e512 + c * BSD);
            const float* buf = ring.next();
            wide_load(PRE, gpre, offw, c);
            strip_zero<BSD>(acc);
            strip_product<BSD, BSPREAD>(acc, DZ, buf, ring, [&](int ct, int j) {
                bfetch_cols(ring, a.w1T[g], c, ct, j);
                if (c == 0) spread_at(gdz, row, DZ, ct, j, 1);
                kg.hook(ct, j);
            });
            const unsigned kb = kg.finish();
            to_regs<BSD>(DP, acc);
            apply_keep(DP, kb, dc.scale);
#pragma unroll
            for (int ct = 0; ct < BNT; ++ct)
#pragma unroll
#ifdef AMID_BS_ABLATE_GELU
                for (int e = 0; e < 4; ++e) DP.v[ct][e] *= PRE.v[ct][e];
#else
                for (int e = 0; e < 4; ++e) DP.v[ct][e] *= gelu_df(PRE.v[ct][e]);
#endif
        }
        {   // dy2 += dpre_c W1_c
            const float* buf = ring.next();
            const float* nxt = c + 1 < BSC ? btile_rows<R>(a.w2T[g], c + 1) : a.woT[g];
            if (c + 1 == BSC) { strip_load<BSD>(X1, GBuf(a.x1, sg.act_bytes), row); gam.load(a.la[g]); }
            if (c == 0) kg.begin(dc, g, SITE_SUB_IN, e128);
            strip_product<BSD, BSPREAD>(accy, DP, buf, ring, [&](int ct, int j) {
                ring.fetch(nxt, ct, j);
                wide_spread(gdpre, offw, c, DP, ct, j, 1);
                if (c == 0) kg.hook(ct, j);
            });
            if (c == 0) kb_in = kg.finish();
        }
    }
    StripRegs<BSD> dgam, dbet;
    {   // dx1 = LNb_out'(dy2 ; x1) + dr ; dt = dx1 * drop_in ; d_o = dt Wo
        const unsigned kb = kb_in;
        to_regs<BSD>(DZ, accy);
        strip_lnb_bwd(DP, DZ, X1, gam, dgam, dbet);
#pragma unroll
        for (int ct = 0; ct < BNT; ++ct) DP.v[ct] += DX2.v[ct];
        DZ = DP;
        apply_keep(DZ, kb, dc.scale);
        const float* buf = ring.next();
        strip_zero<BSD>(acc);
        strip_product<BSD, BSPREAD>(acc, DZ, buf, ring, [&](int ct, int j) { spread_at(gdx1, row, DP, ct, j, 1); spread_at(gdt, row, DZ, ct, j, 3); });
        to_regs<BSD>(PRE, acc);
        strip_store<BSD>(GBuf(a.d_o, sg.act_bytes), row, PRE);
    }
    ln_partials_wave<BSD>(scratch, dgam, dbet);
}

template <int MODE>
__global__ __launch_bounds__(STRIP_THREADS) void bert_strip_ffn_bwd_kernel(const BStripFfnBwdArgs a, const StripGeom sg) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    typename BRingSel<MODE>::type ring(smem);
    ring.first(a.w2T[strip_domain(blockIdx.x)]);
    const StripTile t = strip_tile(sg, blockIdx.x);
    if (!t.live) { zero_slot<BSD>(a.ln_part, t.slot); w_ring_wait(); return; }
    const StripRow row = strip_row<BSD>(sg, t);
    StripRegs<BSD> DX2;
    strip_load<BSD>(DX2, GBuf(a.dx2, sg.act_bytes), row);
    const BDrop dc = bffn_drop(a);          // (the first slab is still landing: these two sites' counters cost no matrix time)
    const unsigned long long e128 = (unsigned long long)row.local * BSD;
    const unsigned kb_block = keep_bits(dc, t.g, SITE_BLOCK, e128), kb_out = keep_bits(dc, t.g, SITE_SUB_OUT, e128);
    bffn_bwd_chain(a, sg, ring, row, t.g, DX2, ln_scratch<BSD>(smem, 0), kb_block, kb_out);
    __syncthreads();
    ln_partials_out<BSD>(ln_scratch<BSD>(smem, 0), a.ln_part + (long long)t.slot * 2 * BSD);
}

// FFN = true: the block below's feed-forward / out-projection backward continues on d x in registers (d x is then never stored)
template <bool FFN, int MODE>
__global__ __launch_bounds__(STRIP_THREADS) void bert_strip_qkv_bwd_kernel(const BStripQkvBwdArgs a, const BStripFfnBwdArgs f, const StripGeom sg) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    if constexpr (!FFN) {
        if ((int)blockIdx.x >= 2 * sg.tpg) { zero_dead_rows(a.dx, sg, blockIdx.x - 2 * sg.tpg, a.zero_blocks); return; }
    }
    typename BRingSel<MODE>::type ring(smem);
    ring.first(a.wT[0][strip_domain(blockIdx.x)]);
    const StripTile t = strip_tile(sg, blockIdx.x);
    if (!t.live) {
        zero_slot<BSD>(a.ln_part, t.slot);
        if constexpr (FFN) zero_slot<BSD>(f.ln_part, t.slot);
        w_ring_wait();
        return;
    }
    const StripRow row = strip_row<BSD>(sg, t);
    const int g = t.g;
    StripRegs<BSD> D0, D1, Xs, DX;
    ColVec<BSD> gam;
    strip_load<BSD>(D0, GBuf(a.dq, sg.act_bytes), row);
    f32x4 acc[BNT];
    strip_zero<BSD>(acc);
    // FFN: the keep bits of the block below's last two dropout sites are drawn under this chain's first two products
    KeepGen kg;
    unsigned kb_block = ~0u, kb_out = ~0u;
    BDrop fdc = {0, 0u, 1.f, 0ull, 0u, 0};
    if constexpr (FFN) fdc = bffn_drop(f);
    const unsigned long long e128 = (unsigned long long)row.local * BSD;
    {   // dq Wq          (every operand is requested one slab ahead of its use)
        if constexpr (FFN) kg.begin(fdc, g, SITE_BLOCK, e128);
        const float* buf = ring.next();
        strip_load<BSD>(D1, GBuf(a.dk, sg.act_bytes), row);
        strip_product<BSD, BSPREAD>(acc, D0, buf, ring, [&](int ct, int j) { ring.fetch(a.wT[1][g], ct, j); if constexpr (FFN) kg.hook(ct, j); });
        if constexpr (FFN) kb_block = kg.finish();
    }
    {   // + dk Wk
        if constexpr (FFN) kg.begin(fdc, g, SITE_SUB_OUT, e128);
        const float* buf = ring.next();
        strip_load<BSD>(D0, GBuf(a.dv, sg.act_bytes), row);
        strip_product<BSD, BSPREAD>(acc, D1, buf, ring, [&](int ct, int j) { ring.fetch(a.wT[2][g], ct, j); if constexpr (FFN) kg.hook(ct, j); });
        if constexpr (FFN) kb_out = kg.finish();
    }
    StripRegs<BSD> dgam, dbet;
    {   // + dv Wv ; dx = LNb_in'(. ; x) + dx1
        const float* buf = ring.next();
        strip_load<BSD>(Xs, GBuf(a.x, sg.act_bytes), row);
        strip_load<BSD>(D1, GBuf(a.dx1, sg.act_bytes), row);
        gam.load(a.la[g]);
        strip_product<BSD, BSPREAD>(acc, D0, buf, ring, [&](int ct, int j) { if constexpr (FFN) ring.fetch(f.w2T[g], ct, j); });
        to_regs<BSD>(D0, acc);
        strip_lnb_bwd(DX, D0, Xs, gam, dgam, dbet);
#pragma unroll
        for (int ct = 0; ct < BNT; ++ct) DX.v[ct] += D1.v[ct];
    }
    ln_partials_wave<BSD>(ln_scratch<BSD>(smem, 0), dgam, dbet);
    if constexpr (FFN) {
        bffn_bwd_chain(f, sg, ring, row, g, DX, ln_scratch<BSD>(smem, 1), kb_block, kb_out);
    } else {
        strip_store<BSD>(GBuf(a.dx, sg.act_bytes), row, DX);
    }
    __syncthreads();
    ln_partials_out<BSD>(ln_scratch<BSD>(smem, 0), a.ln_part + (long long)t.slot * 2 * BSD);
    if constexpr (FFN) ln_partials_out<BSD>(ln_scratch<BSD>(smem, 1), f.ln_part + (long long)t.slot * 2 * BSD);
}

}  // namespace amid

using namespace amid;
using namespace amid_strip_host;

// the 512-wide tensors go through buffer descriptors too: 4 x the bytes of a [2M, 128] tensor must stay below 2 GiB
static int bert_strip_geom(int B, int T, const int* live, StripGeom* sg) {
    if (int e = make_strip_geom(B, T, BSD, live, sg)) return e;
    if (4LL * sg->act_bytes > 0x7FFFFFF0LL) return AMID_ERR_UNSUPPORTED;
    return AMID_OK;
}

// 1 when the strip kernels cover the shape (hidden 128; activations [2 B T, 512] fp32 within 2 GiB); the caller falls back to the
// row-tile kernels of bert.hip otherwise
extern "C" int amid_bert_strip_supported(int B, int T, int D) {
    return (D == BSD && B > 0 && T > 0 && 2LL * B * T * BSF * 4 <= 0x7FFFFFF0LL) ? 1 : 0;
}

static void fill_bqkv(BStripQkvArgs& a, const float* x, const float* const* la, const float* const* lb, const float* const* w3,
                      const float* const* b3, float* y, float* q, float* k, float* v) {
    a.x = x; a.y = y; a.out[0] = q; a.out[1] = k; a.out[2] = v;
    for (int g = 0; g < 2; ++g) {
        a.la[g] = la[g]; a.lb[g] = lb[g];
        for (int j = 0; j < 3; ++j) { a.w[j][g] = w3[j * 2 + g]; a.b[j][g] = b3[j * 2 + g]; }
    }
}

static int bqkv_fwd(const float* x, const float* const* la, const float* const* lb, const float* const* w3, const float* const* b3, int B,
                    int T, const int* live, float* y, float* q, float* k, float* v, const BPrologue& pro, void* stream, int mode = 0) {
    AMID_CHECK_ARG(x && la && lb && w3 && b3 && q && k && v);       // (y == NULL: not stored)
    BStripQkvArgs a;
    fill_bqkv(a, x, la, lb, w3, b3, y, q, k, v);
    StripGeom sg;
    if (int e = bert_strip_geom(B, T, live, &sg)) return e;
    static unsigned long long attr_done[2] = {0, 0};
    if (mode == 3) {
        if (int rc = lds_attr_once((const void*)bert_strip_qkv_fwd_kernel<3>, strip_lds_bytes<BSD>(), attr_done[1])) return rc;
        bert_strip_qkv_fwd_kernel<3><<<2 * sg.tpg + pro.blocks, STRIP_THREADS, strip_lds_bytes<BSD>(), (hipStream_t)stream>>>(a, sg, pro);
    } else {
        if (int rc = lds_attr_once((const void*)bert_strip_qkv_fwd_kernel<0>, strip_lds_bytes<BSD>(), attr_done[0])) return rc;
        bert_strip_qkv_fwd_kernel<0><<<2 * sg.tpg + pro.blocks, STRIP_THREADS, strip_lds_bytes<BSD>(), (hipStream_t)stream>>>(a, sg, pro);
    }
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? AMID_OK : (int)e;
}

// w3 / b3: host arrays of six device pointers ordered [q, k, v][domain] (as amid_bert_qkv_fwd_f32).  y == NULL: LNb_in(x) is not stored (an
// inference forward: nobody reads it)
extern "C" int amid_bert_strip_qkv_fwd_f32(const float* x, const float* const* la, const float* const* lb, const float* const* w3,
                                           const float* const* b3, int B, int T, const int* live, float* y, float* q, float* k, float* v,
                                           void* stream) {
    BPrologue pro = {};
    return bqkv_fwd(x, la, lb, w3, b3, B, T, live, y, q, k, v, pro, stream);
}

// ... with the step's prologue riding as extra workgroups: key_keep[i] = seq_d2[i] > 0 for i < n_keys (seq_d2 == NULL: none), and
// tr_dst[m][c][r] = tr_src[m][r][c] for n_tr <= 24 matrices of tr_rows[m] x tr_cols[m] floats (multiples of 64) -- what
// amid_key_keep_u8 and amid_transpose_rect_f32 do in launches of their own
static int bqkv_fwd_pro(const float* x, const float* const* la, const float* const* lb, const float* const* w3,
                        const float* const* b3, int B, int T, const int* live, float* y, float* q, float* k,
                        float* v, const long long* seq_d2, int n_keys, unsigned char* key_keep,
                        const float* const* tr_src, float* const* tr_dst, const int* tr_rows, const int* tr_cols,
                        int n_tr, void* stream, int mode) {
    AMID_CHECK_ARG(n_tr >= 0 && n_tr <= BPRO_MAX && (n_tr == 0 || (tr_src && tr_dst && tr_rows && tr_cols)));
    AMID_CHECK_ARG(seq_d2 == nullptr || (key_keep != nullptr && n_keys > 0));
    BPrologue pro = {};
    pro.seq = seq_d2; pro.keep = key_keep; pro.n_keys = n_keys; pro.n = n_tr;
    for (int i = 0; i < n_tr; ++i) {
        AMID_CHECK_ARG(tr_src[i] && tr_dst[i] && tr_rows[i] > 0 && tr_cols[i] > 0 && tr_rows[i] % 64 == 0 && tr_cols[i] % 64 == 0);
        pro.src[i] = tr_src[i]; pro.dst[i] = tr_dst[i]; pro.rows[i] = tr_rows[i]; pro.cols[i] = tr_cols[i];
    }
    pro.blocks = (seq_d2 != nullptr || n_tr > 0) ? 96 : 0;
    return bqkv_fwd(x, la, lb, w3, b3, B, T, live, y, q, k, v, pro, stream, mode);
}
extern "C" int amid_bert_strip_qkv_fwd_pro_f32(const float* x, const float* const* la, const float* const* lb, const float* const* w3,
                                               const float* const* b3, int B, int T, const int* live, float* y, float* q, float* k,
                                               float* v, const long long* seq_d2, int n_keys, unsigned char* key_keep,
                                               const float* const* tr_src, float* const* tr_dst, const int* tr_rows, const int* tr_cols,
                                               int n_tr, void* stream) {
    return bqkv_fwd_pro(x, la, lb, w3, b3, B, T, live, y, q, k, v, seq_d2, n_keys, key_keep, tr_src, tr_dst, tr_rows, tr_cols, n_tr, stream, 0);
}
// ... on bf16 pieces: w3 = the tiles' three-plane images (amid_bert_weight_images_f32), everything else as above
extern "C" int amid_bert_strip_qkv_fwd_pro_p3_f32(const float* x, const float* const* la, const float* const* lb, const float* const* w3_img,
                                                  const float* const* b3, int B, int T, const int* live, float* y, float* q, float* k,
                                                  float* v, const long long* seq_d2, int n_keys, unsigned char* key_keep,
                                                  const float* const* tr_src, float* const* tr_dst, const int* tr_rows, const int* tr_cols,
                                                  int n_tr, void* stream) {
    return bqkv_fwd_pro(x, la, lb, w3_img, b3, B, T, live, y, q, k, v, seq_d2, n_keys, key_keep, tr_src, tr_dst, tr_rows, tr_cols, n_tr, stream, 3);
}

// out-projection + feed-forward of a block; nla != NULL: the next block's LayerNorm + q / k / v on x2 in the same launch (x2 is
// then also the next block's saved input).  x1, y2, pre, h, ny: each may be NULL = not stored (an inference forward)
static int boproj_ffn_fwd(const float* o, const float* x, const float* const* wo, const float* const* bo,
                          const float* const* la, const float* const* lb, const float* const* w1,
                          const float* const* b1, const float* const* w2, const float* const* b2, int B, int T,
                          const int* live, int layer, const void* step_state, int train, float p_drop, float* x1,
                          float* y2, float* pre, float* h, float* x2, const float* const* nla,
                          const float* const* nlb, const float* const* nw3, const float* const* nb3, float* ny,
                          float* nq, float* nk, float* nv, void* stream, int mode) {
    AMID_CHECK_ARG(o && x && wo && bo && la && lb && w1 && b1 && w2 && b2 && x2 && (!train || step_state));      // (x1, y2, pre, h == NULL: not stored)
    const bool next = nla != nullptr;
    AMID_CHECK_ARG(!next || (nlb && nw3 && nb3 && nq && nk && nv));
    BStripOffArgs a;
    a.o = o; a.x = x; a.x1 = x1; a.y2 = y2; a.pre = pre; a.h = h; a.x2 = x2;
    a.st = (const StepState*)step_state; a.layer = layer;
    a.train = (train && p_drop > 0.f) ? 1 : 0;
    a.spec = drop_spec(p_drop);
    if (a.train && spec_bits(a.spec) != 16) return AMID_ERR_UNSUPPORTED;      // KeepGen: the 16-bit decisions of p = 0.1 (the reference's rate, model_seq.py:267)
    a.scale = a.train ? 1.0f / (1.0f - p_drop) : 1.0f;
    for (int g = 0; g < 2; ++g) {
        a.wo[g] = wo[g]; a.bo[g] = bo[g]; a.la[g] = la[g]; a.lb[g] = lb[g];
        a.w1[g] = w1[g]; a.b1[g] = b1[g]; a.w2[g] = w2[g]; a.b2[g] = b2[g];
    }
    BStripQkvArgs nx = {};
    if (next) fill_bqkv(nx, x2, nla, nlb, nw3, nb3, ny, nq, nk, nv);
    StripGeom sg;
    if (int e = bert_strip_geom(B, T, live, &sg)) return e;
    if (mode == 3)
        return next ? launch_strip<bert_strip_oproj_ffn_fwd_kernel<true, 3>, BSD>(sg, stream, a, nx)
                    : launch_strip<bert_strip_oproj_ffn_fwd_kernel<false, 3>, BSD>(sg, stream, a, nx);
    return next ? launch_strip<bert_strip_oproj_ffn_fwd_kernel<true, 0>, BSD>(sg, stream, a, nx)
                : launch_strip<bert_strip_oproj_ffn_fwd_kernel<false, 0>, BSD>(sg, stream, a, nx);
}
extern "C" int amid_bert_strip_oproj_ffn_fwd_f32(const float* o, const float* x, const float* const* wo, const float* const* bo,
                                                 const float* const* la, const float* const* lb, const float* const* w1,
                                                 const float* const* b1, const float* const* w2, const float* const* b2, int B, int T,
                                                 const int* live, int layer, const void* step_state, int train, float p_drop, float* x1,
                                                 float* y2, float* pre, float* h, float* x2, const float* const* nla,
                                                 const float* const* nlb, const float* const* nw3, const float* const* nb3, float* ny,
                                                 float* nq, float* nk, float* nv, void* stream) {
    return boproj_ffn_fwd(o, x, wo, bo, la, lb, w1, b1, w2, b2, B, T, live, layer, step_state, train, p_drop, x1, y2, pre, h, x2, nla, nlb, nw3, nb3,
                          ny, nq, nk, nv, stream, 0);
}
// ... on bf16 pieces: wo / nw3 = tile images, w1 / w2 = the first of their four tiles' images (one behind the other)
extern "C" int amid_bert_strip_oproj_ffn_fwd_p3_f32(const float* o, const float* x, const float* const* wo_img, const float* const* bo,
                                                    const float* const* la, const float* const* lb, const float* const* w1_img,
                                                    const float* const* b1, const float* const* w2_img, const float* const* b2, int B, int T,
                                                    const int* live, int layer, const void* step_state, int train, float p_drop, float* x1,
                                                    float* y2, float* pre, float* h, float* x2, const float* const* nla,
                                                    const float* const* nlb, const float* const* nw3_img, const float* const* nb3, float* ny,
                                                    float* nq, float* nk, float* nv, void* stream) {
    return boproj_ffn_fwd(o, x, wo_img, bo, la, lb, w1_img, b1, w2_img, b2, B, T, live, layer, step_state, train, p_drop, x1, y2, pre, h, x2, nla, nlb,
                          nw3_img, nb3, ny, nq, nk, nv, stream, 3);
}

static int fill_bffn_bwd(BStripFfnBwdArgs& a, const float* dx2, const float* pre, const float* x1, const float* const* la,
                         const float* const* w2T, const float* const* w1T, const float* const* woT, int layer, const void* step_state,
                         int train, float p_drop, float* dz, float* dpre, float* dx1, float* dt, float* d_o, float* ln_part) {
    AMID_CHECK_ARG(pre && x1 && la && w2T && w1T && woT && dz && dpre && dx1 && dt && d_o && ln_part && (!train || step_state));
    a.dx2 = dx2; a.pre = pre; a.x1 = x1; a.dz = dz; a.dpre = dpre; a.dx1 = dx1; a.dt = dt; a.d_o = d_o; a.ln_part = ln_part;
    a.st = (const StepState*)step_state; a.layer = layer;
    a.train = (train && p_drop > 0.f) ? 1 : 0;
    a.spec = drop_spec(p_drop);
    if (a.train && spec_bits(a.spec) != 16) return AMID_ERR_UNSUPPORTED;
    a.scale = a.train ? 1.0f / (1.0f - p_drop) : 1.0f;
    for (int g = 0; g < 2; ++g) { a.la[g] = la[g]; a.w2T[g] = w2T[g]; a.w1T[g] = w1T[g]; a.woT[g] = woT[g]; }
    return AMID_OK;
}

// ln_part: [2 * ceil(B T / amid_sas_strip_tile_rows())][2][128]; domain g's partial sums are slots [g * tpg, (g + 1) * tpg)
static int bffn_bwd(const float* dx2, const float* pre, const float* x1, const float* const* la,
                    const float* const* w2T, const float* const* w1T, const float* const* woT, int B, int T,
                    const int* live, int layer, const void* step_state, int train, float p_drop, float* dz,
                    float* dpre, float* dx1, float* dt, float* d_o, float* ln_part, void* stream, int mode) {
    AMID_CHECK_ARG(dx2);
    BStripFfnBwdArgs a;
    if (int e = fill_bffn_bwd(a, dx2, pre, x1, la, w2T, w1T, woT, layer, step_state, train, p_drop, dz, dpre, dx1, dt, d_o, ln_part)) return e;
    StripGeom sg;
    if (int e = bert_strip_geom(B, T, live, &sg)) return e;
    return mode == 3 ? launch_strip<bert_strip_ffn_bwd_kernel<3>, BSD>(sg, stream, a) : launch_strip<bert_strip_ffn_bwd_kernel<0>, BSD>(sg, stream, a);
}
extern "C" int amid_bert_strip_ffn_bwd_f32(const float* dx2, const float* pre, const float* x1, const float* const* la,
                                           const float* const* w2T, const float* const* w1T, const float* const* woT, int B, int T,
                                           const int* live, int layer, const void* step_state, int train, float p_drop, float* dz,
                                           float* dpre, float* dx1, float* dt, float* d_o, float* ln_part, void* stream) {
    return bffn_bwd(dx2, pre, x1, la, w2T, w1T, woT, B, T, live, layer, step_state, train, p_drop, dz, dpre, dx1, dt, d_o, ln_part, stream, 0);
}
// ... on bf16 pieces: w2T / w1T = the first of the four TRANSPOSED tiles' images, woT = the transposed tile's image
extern "C" int amid_bert_strip_ffn_bwd_p3_f32(const float* dx2, const float* pre, const float* x1, const float* const* la,
                                              const float* const* w2T_img, const float* const* w1T_img, const float* const* woT_img, int B, int T,
                                              const int* live, int layer, const void* step_state, int train, float p_drop, float* dz,
                                              float* dpre, float* dx1, float* dt, float* d_o, float* ln_part, void* stream) {
    return bffn_bwd(dx2, pre, x1, la, w2T_img, w1T_img, woT_img, B, T, live, layer, step_state, train, p_drop, dz, dpre, dx1, dt, d_o, ln_part, stream, 3);
}

// wT3: six device pointers ordered [q, k, v][domain] (transposed weights).  fpre != NULL: the block below's feed-forward /
// out-projection backward (f* arguments, as amid_bert_strip_ffn_bwd_f32 without dx2) runs on d x in the same launch; dx is then not written.
// zero_dead (with a live list and dx): the rows of dx that belong to the sequences NOT on the list are zero-filled by extra workgroups
static int bqkv_bwd(const float* dq, const float* dk, const float* dv, const float* dx1, const float* x,
                    const float* const* la, const float* const* wT3, int B, int T, const int* live, float* dx,
                    int zero_dead, float* ln_part, const float* fpre, const float* fx1, const float* const* fla,
                    const float* const* fw2T, const float* const* fw1T, const float* const* fwoT, int flayer,
                    const void* step_state, int train, float p_drop, float* fdz, float* fdpre, float* fdx1,
                    float* fdt, float* fd_o, float* fln_part, void* stream, int mode) {
    AMID_CHECK_ARG(dq && dk && dv && dx1 && x && la && wT3 && ln_part);
    const bool ffn = fpre != nullptr;
    AMID_CHECK_ARG(ffn || dx);
    BStripQkvBwdArgs a;
    a.dq = dq; a.dk = dk; a.dv = dv; a.dx1 = dx1; a.x = x; a.dx = dx; a.ln_part = ln_part;
    for (int g = 0; g < 2; ++g) {
        a.la[g] = la[g];
        for (int j = 0; j < 3; ++j) a.wT[j][g] = wT3[j * 2 + g];
    }
    BStripFfnBwdArgs f = {};
    if (ffn) if (int e = fill_bffn_bwd(f, nullptr, fpre, fx1, fla, fw2T, fw1T, fwoT, flayer, step_state, train, p_drop, fdz, fdpre, fdx1, fdt, fd_o, fln_part)) return e;
    StripGeom sg;
    if (int e = bert_strip_geom(B, T, live, &sg)) return e;
    a.zero_blocks = (zero_dead && live != nullptr && !ffn) ? (B < 256 ? B : 256) : 0;
    if (ffn) return mode == 3 ? launch_strip<bert_strip_qkv_bwd_kernel<true, 3>, BSD>(sg, stream, a, f)
                              : launch_strip<bert_strip_qkv_bwd_kernel<true, 0>, BSD>(sg, stream, a, f);
    static unsigned long long attr_done[2] = {0, 0};
    if (mode == 3) {
        if (int rc = lds_attr_once((const void*)bert_strip_qkv_bwd_kernel<false, 3>, strip_lds_bytes<BSD>(), attr_done[1])) return rc;
        bert_strip_qkv_bwd_kernel<false, 3><<<2 * sg.tpg + a.zero_blocks, STRIP_THREADS, strip_lds_bytes<BSD>(), (hipStream_t)stream>>>(a, f, sg);
    } else {
        if (int rc = lds_attr_once((const void*)bert_strip_qkv_bwd_kernel<false, 0>, strip_lds_bytes<BSD>(), attr_done[0])) return rc;
        bert_strip_qkv_bwd_kernel<false, 0><<<2 * sg.tpg + a.zero_blocks, STRIP_THREADS, strip_lds_bytes<BSD>(), (hipStream_t)stream>>>(a, f, sg);
    }
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? AMID_OK : (int)e;
}
extern "C" int amid_bert_strip_qkv_bwd_f32(const float* dq, const float* dk, const float* dv, const float* dx1, const float* x,
                                           const float* const* la, const float* const* wT3, int B, int T, const int* live, float* dx,
                                           int zero_dead, float* ln_part, const float* fpre, const float* fx1, const float* const* fla,
                                           const float* const* fw2T, const float* const* fw1T, const float* const* fwoT, int flayer,
                                           const void* step_state, int train, float p_drop, float* fdz, float* fdpre, float* fdx1,
                                           float* fdt, float* fd_o, float* fln_part, void* stream) {
    return bqkv_bwd(dq, dk, dv, dx1, x, la, wT3, B, T, live, dx, zero_dead, ln_part, fpre, fx1, fla, fw2T, fw1T, fwoT, flayer, step_state, train, p_drop,
                    fdz, fdpre, fdx1, fdt, fd_o, fln_part, stream, 0);
}
// ... on bf16 pieces: every weight argument = transposed tile images (as amid_bert_strip_ffn_bwd_p3_f32)
extern "C" int amid_bert_strip_qkv_bwd_p3_f32(const float* dq, const float* dk, const float* dv, const float* dx1, const float* x,
                                              const float* const* la, const float* const* wT3_img, int B, int T, const int* live, float* dx,
                                              int zero_dead, float* ln_part, const float* fpre, const float* fx1, const float* const* fla,
                                              const float* const* fw2T_img, const float* const* fw1T_img, const float* const* fwoT_img, int flayer,
                                              const void* step_state, int train, float p_drop, float* fdz, float* fdpre, float* fdx1,
                                              float* fdt, float* fd_o, float* fln_part, void* stream) {
    return bqkv_bwd(dq, dk, dv, dx1, x, la, wT3_img, B, T, live, dx, zero_dead, ln_part, fpre, fx1, fla, fw2T_img, fw1T_img, fwoT_img, flayer, step_state,
                    train, p_drop, fdz, fdpre, fdx1, fdt, fd_o, fln_part, stream, 3);
}

// Three-plane bf16 fragment images (weights_image.h: hi + mid + lo = the fp32 element exactly) of n <= 96 weight TILES of 128 x 128: tile i
// is src[i][r * ld[i] + c] (tr[i] = 0) or its transpose src[i][c * ld[i] + r] (tr[i] != 0), r, c < 128; dst16: [n][3][128][128] bf16.
// One launch per step in front of the first strip launch (what SASRec's gather carries as riders).
constexpr int BIMG_MAX = 96;
struct BImgArgs { const float* src[BIMG_MAX]; unsigned short ld[BIMG_MAX]; unsigned char tr[BIMG_MAX]; int n, per; unsigned short* dst; };
__global__ __launch_bounds__(256) void bert_weight_images_kernel(const BImgArgs a) {
    const int wi = blockIdx.x / a.per, b = blockIdx.x - wi * a.per;
    weights_image_block(a.src[wi], a.dst + (size_t)wi * 3 * BSD * BSD, BSD, a.tr[wi], 3, b, a.per, a.ld[wi]);
}
extern "C" int amid_bert_weight_images_f32(const float* const* src, const int* ld, const int* tr, int n, void* dst16, void* stream) {
    AMID_CHECK_ARG(src && ld && tr && dst16 && n > 0 && n <= BIMG_MAX);
    BImgArgs a;
    for (int i = 0; i < n; ++i) {
        AMID_CHECK_ARG(src[i] && ld[i] >= BSD && ld[i] < 65536);
        a.src[i] = src[i]; a.ld[i] = (unsigned short)ld[i]; a.tr[i] = tr[i] ? 1 : 0;
    }
    a.n = n; a.per = 4; a.dst = (unsigned short*)dst16;
    bert_weight_images_kernel<<<n * a.per, 256, 0, (hipStream_t)stream>>>(a);
    AMID_LAUNCH_CHECK();
    return AMID_OK;
}
