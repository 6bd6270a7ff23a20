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

// how a launch multiplies: fp32 matrix instructions on the fp32 weights, or fp32 operands as three bf16 pieces on the weights' three-plane
// tile images (amid_bert_weight_images_f32; the *_p3_f32 entries) -- the values are the kernels' MODE
enum BProducts { B_FP32 = 0, B_PIECES3 = 3 };

// LayerNorm + q / k / v of a block as its entries state it (every field null / zero unless named).  w3 / b3: host arrays of six device
// pointers ordered [q, k, v][domain] (as amid_bert_qkv_fwd_f32).  y == NULL: LNb_in(x) is not stored (an inference forward: nobody reads it).
// Optional, the step's prologue riding as extra workgroups: key_keep[i] = seq_d2[i] > 0 for i < n_keys (seq_d2 == NULL: none), and
// tr_dst[m][c][r] = tr_src[m][r][c] for n_tr <= 24 matrices of tr_rows[m] x tr_cols[m] floats (multiples of 64) -- what amid_key_keep_u8 and
// amid_transpose_rect_f32 do in launches of their own
struct BQkvFwdCall {
    const float* x = nullptr; FamC la = nullptr, lb = nullptr, w3 = nullptr, b3 = nullptr;
    int B = 0, T = 0; const int* live = nullptr;
    float* y = nullptr; float* q = nullptr; float* k = nullptr; float* v = nullptr;
    const long long* seq_d2 = nullptr; int n_keys = 0; unsigned char* key_keep = nullptr;
    FamC tr_src = nullptr; Fam tr_dst = nullptr; const int* tr_rows = nullptr; const int* tr_cols = nullptr; int n_tr = 0;
    BProducts products = B_FP32; void* stream = nullptr;
};
#define BQKV_FWD_CALL(c, w3_) BQkvFwdCall c; c.x = x; c.la = la; c.lb = lb; c.w3 = w3_; c.b3 = b3; c.B = B; c.T = T; c.live = live; c.y = y; c.q = q; c.k = k; c.v = v; c.stream = stream
#define BQKV_FWD_PRO(c)                                                                                                                         \
    c.seq_d2 = seq_d2; c.n_keys = n_keys; c.key_keep = key_keep; c.tr_src = tr_src; c.tr_dst = tr_dst; c.tr_rows = tr_rows; c.tr_cols = tr_cols; \
    c.n_tr = n_tr

static int bqkv_fwd(const BQkvFwdCall& c) {
    AMID_CHECK_ARG(c.n_tr >= 0 && c.n_tr <= BPRO_MAX && (c.n_tr == 0 || (c.tr_src && c.tr_dst && c.tr_rows && c.tr_cols)));
    AMID_CHECK_ARG(c.seq_d2 == nullptr || (c.key_keep != nullptr && c.n_keys > 0));
    BPrologue pro = {};
    pro.seq = c.seq_d2; pro.keep = c.key_keep; pro.n_keys = c.n_keys; pro.n = c.n_tr;
    for (int i = 0; i < c.n_tr; ++i) {
        AMID_CHECK_ARG(c.tr_src[i] && c.tr_dst[i] && c.tr_rows[i] > 0 && c.tr_cols[i] > 0 && c.tr_rows[i] % 64 == 0 && c.tr_cols[i] % 64 == 0);
        pro.src[i] = c.tr_src[i]; pro.dst[i] = c.tr_dst[i]; pro.rows[i] = c.tr_rows[i]; pro.cols[i] = c.tr_cols[i];
    }
    pro.blocks = (c.seq_d2 != nullptr || c.n_tr > 0) ? 96 : 0;
    AMID_CHECK_ARG(c.x && c.la && c.lb && c.w3 && c.b3 && c.q && c.k && c.v);       // (y == NULL: not stored)
    BStripQkvArgs a;
    fill_bqkv(a, c.x, c.la, c.lb, c.w3, c.b3, c.y, c.q, c.k, c.v);
    StripGeom sg;
    if (int e = bert_strip_geom(c.B, c.T, c.live, &sg)) return e;
    const int grid = 2 * sg.tpg + pro.blocks;
    return c.products == B_PIECES3 ? launch_lds<bert_strip_qkv_fwd_kernel<3>>(grid, STRIP_THREADS, strip_lds_bytes<BSD>(), c.stream, a, sg, pro)
                                   : launch_lds<bert_strip_qkv_fwd_kernel<0>>(grid, STRIP_THREADS, strip_lds_bytes<BSD>(), c.stream, a, sg, pro);
}

extern "C" int amid_bert_strip_qkv_fwd_f32(const float* x, const float* const* la, const float* const* lb, const float* const* w3,
                                           const float* const* b3, int B, int T, const int* live, float* y, float* q, float* k, float* v,
                                           void* stream) {
    BQKV_FWD_CALL(c, w3);
    return bqkv_fwd(c);
}
extern "C" int amid_bert_strip_qkv_fwd_pro_f32(const float* x, const float* const* la, const float* const* lb, const float* const* w3,
                                               const float* const* b3, int B, int T, const int* live, float* y, float* q, float* k,
                                               float* v, const long long* seq_d2, int n_keys, unsigned char* key_keep,
                                               const float* const* tr_src, float* const* tr_dst, const int* tr_rows, const int* tr_cols,
                                               int n_tr, void* stream) {
    BQKV_FWD_CALL(c, w3); BQKV_FWD_PRO(c);
    return bqkv_fwd(c);
}
// ... on bf16 pieces: w3 = the tiles' three-plane images (amid_bert_weight_images_f32), everything else as above
extern "C" int amid_bert_strip_qkv_fwd_pro_p3_f32(const float* x, const float* const* la, const float* const* lb, const float* const* w3_img,
                                                  const float* const* b3, int B, int T, const int* live, float* y, float* q, float* k,
                                                  float* v, const long long* seq_d2, int n_keys, unsigned char* key_keep,
                                                  const float* const* tr_src, float* const* tr_dst, const int* tr_rows, const int* tr_cols,
                                                  int n_tr, void* stream) {
    BQKV_FWD_CALL(c, w3_img); BQKV_FWD_PRO(c); c.products = B_PIECES3;
    return bqkv_fwd(c);
}
#undef BQKV_FWD_PRO
#undef BQKV_FWD_CALL

// out-projection + feed-forward of a block; nla != NULL: the next block's LayerNorm + q / k / v on x2 in the same launch (x2 is
// then also the next block's saved input).  x1, y2, pre, h, ny: each may be NULL = not stored (an inference forward)
struct BOffCall {
    const float* o = nullptr; const float* x = nullptr;
    FamC wo = nullptr, bo = nullptr, la = nullptr, lb = nullptr, w1 = nullptr, b1 = nullptr, w2 = nullptr, b2 = nullptr;
    int B = 0, T = 0; const int* live = nullptr;
    int layer = 0; const void* step_state = nullptr; int train = 0; float p_drop = 0.f;
    float* x1 = nullptr; float* y2 = nullptr; float* pre = nullptr; float* h = nullptr; float* x2 = nullptr;
    FamC nla = nullptr, nlb = nullptr, nw3 = nullptr, nb3 = nullptr;
    float* ny = nullptr; float* nq = nullptr; float* nk = nullptr; float* nv = nullptr;
    BProducts products = B_FP32; void* stream = nullptr;
};
#define BOFF_CALL(c, wo_, w1_, w2_, nw3_)                                                                                                       \
    BOffCall c;                                                                                                                                 \
    c.o = o; c.x = x; c.wo = wo_; c.bo = bo; c.la = la; c.lb = lb; c.w1 = w1_; c.b1 = b1; c.w2 = w2_; c.b2 = b2; c.B = B; c.T = T; c.live = live;   \
    c.layer = layer; c.step_state = step_state; c.train = train; c.p_drop = p_drop; c.x1 = x1; c.y2 = y2; c.pre = pre; c.h = h; c.x2 = x2;       \
    c.nla = nla; c.nlb = nlb; c.nw3 = nw3_; c.nb3 = nb3; c.ny = ny; c.nq = nq; c.nk = nk; c.nv = nv; c.stream = stream

static int boproj_ffn_fwd(const BOffCall& c) {
    AMID_CHECK_ARG(c.o && c.x && c.wo && c.bo && c.la && c.lb && c.w1 && c.b1 && c.w2 && c.b2 && c.x2 && (!c.train || c.step_state));      // (x1, y2, pre, h == NULL: not stored)
    const bool next = c.nla != nullptr;
    AMID_CHECK_ARG(!next || (c.nlb && c.nw3 && c.nb3 && c.nq && c.nk && c.nv));
    BStripOffArgs a;
    a.o = c.o; a.x = c.x; a.x1 = c.x1; a.y2 = c.y2; a.pre = c.pre; a.h = c.h; a.x2 = c.x2;
    a.st = (const StepState*)c.step_state; a.layer = c.layer;
    const DropoutArgs d = dropout_args(c.train, c.p_drop);
    a.train = d.train; a.spec = d.spec; a.scale = d.scale;
    if (a.train && spec_bits(a.spec) != 16) return AMID_ERR_UNSUPPORTED;      // KeepGen: the 16-bit decisions of p = 0.1 (the reference's rate, model_seq.py:267)
    for (int g = 0; g < 2; ++g) {
        a.wo[g] = c.wo[g]; a.bo[g] = c.bo[g]; a.la[g] = c.la[g]; a.lb[g] = c.lb[g];
        a.w1[g] = c.w1[g]; a.b1[g] = c.b1[g]; a.w2[g] = c.w2[g]; a.b2[g] = c.b2[g];
    }
    BStripQkvArgs nx = {};
    if (next) fill_bqkv(nx, c.x2, c.nla, c.nlb, c.nw3, c.nb3, c.ny, c.nq, c.nk, c.nv);
    StripGeom sg;
    if (int e = bert_strip_geom(c.B, c.T, c.live, &sg)) return e;
    if (c.products == B_PIECES3)
        return next ? launch_strip<bert_strip_oproj_ffn_fwd_kernel<true, 3>, BSD>(sg, c.stream, a, nx)
                    : launch_strip<bert_strip_oproj_ffn_fwd_kernel<false, 3>, BSD>(sg, c.stream, a, nx);
    return next ? launch_strip<bert_strip_oproj_ffn_fwd_kernel<true, 0>, BSD>(sg, c.stream, a, nx)
                : launch_strip<bert_strip_oproj_ffn_fwd_kernel<false, 0>, BSD>(sg, c.stream, a, nx);
}
extern "C" int amid_bert_strip_oproj_ffn_fwd_f32(const float* o, const float* x, const float* const* wo, const float* const* bo,
                                                 const float* const* la, const float* const* lb, const float* const* w1,
                                                 const float* const* b1, const float* const* w2, const float* const* b2, int B, int T,
                                                 const int* live, int layer, const void* step_state, int train, float p_drop, float* x1,
                                                 float* y2, float* pre, float* h, float* x2, const float* const* nla,
                                                 const float* const* nlb, const float* const* nw3, const float* const* nb3, float* ny,
                                                 float* nq, float* nk, float* nv, void* stream) {
    BOFF_CALL(c, wo, w1, w2, nw3);
    return boproj_ffn_fwd(c);
}
// ... on bf16 pieces: wo / nw3 = tile images, w1 / w2 = the first of their four tiles' images (one behind the other)
extern "C" int amid_bert_strip_oproj_ffn_fwd_p3_f32(const float* o, const float* x, const float* const* wo_img, const float* const* bo,
                                                    const float* const* la, const float* const* lb, const float* const* w1_img,
                                                    const float* const* b1, const float* const* w2_img, const float* const* b2, int B, int T,
                                                    const int* live, int layer, const void* step_state, int train, float p_drop, float* x1,
                                                    float* y2, float* pre, float* h, float* x2, const float* const* nla,
                                                    const float* const* nlb, const float* const* nw3_img, const float* const* nb3, float* ny,
                                                    float* nq, float* nk, float* nv, void* stream) {
    BOFF_CALL(c, wo_img, w1_img, w2_img, nw3_img); c.products = B_PIECES3;
    return boproj_ffn_fwd(c);
}
#undef BOFF_CALL

// the feed-forward / out-projection backward of a block as an entry states it; inside BQkvBwdCall the optional fused block (absent: pre == NULL)
struct BFfnBwdCall {
    const float* dx2 = nullptr; const float* pre = nullptr; const float* x1 = nullptr;
    FamC la = nullptr, w2T = nullptr, w1T = nullptr, woT = nullptr;
    int layer = 0; const void* step_state = nullptr; int train = 0; float p_drop = 0.f;
    float* dz = nullptr; float* dpre = nullptr; float* dx1 = nullptr; float* dt = nullptr; float* d_o = nullptr; float* ln_part = nullptr;
};
// what every backward strip launch of a block is given besides its operands
struct BBwdLaunch { int B = 0, T = 0; const int* live = nullptr; BProducts products = B_FP32; void* stream = nullptr; };
#define BBWD_LAUNCH(l, products_) BBwdLaunch l; l.B = B; l.T = T; l.live = live; l.products = products_; l.stream = stream

static int fill_bffn_bwd(BStripFfnBwdArgs& a, const BFfnBwdCall& c) {
    AMID_CHECK_ARG(c.pre && c.x1 && c.la && c.w2T && c.w1T && c.woT && c.dz && c.dpre && c.dx1 && c.dt && c.d_o && c.ln_part && (!c.train || c.step_state));
    a.dx2 = c.dx2; a.pre = c.pre; a.x1 = c.x1; a.dz = c.dz; a.dpre = c.dpre; a.dx1 = c.dx1; a.dt = c.dt; a.d_o = c.d_o; a.ln_part = c.ln_part;
    a.st = (const StepState*)c.step_state; a.layer = c.layer;
    const DropoutArgs d = dropout_args(c.train, c.p_drop);
    a.train = d.train; a.spec = d.spec; a.scale = d.scale;
    if (a.train && spec_bits(a.spec) != 16) return AMID_ERR_UNSUPPORTED;
    for (int g = 0; g < 2; ++g) { a.la[g] = c.la[g]; a.w2T[g] = c.w2T[g]; a.w1T[g] = c.w1T[g]; a.woT[g] = c.woT[g]; }
    return AMID_OK;
}

// ln_part: [2 * ceil(B T / amid_sas_strip_tile_rows())][2][128]; domain g's partial sums are slots [g * tpg, (g + 1) * tpg)
static int bffn_bwd(const BFfnBwdCall& c, const BBwdLaunch& l) {
    AMID_CHECK_ARG(c.dx2);
    BStripFfnBwdArgs a;
    if (int e = fill_bffn_bwd(a, c)) return e;
    StripGeom sg;
    if (int e = bert_strip_geom(l.B, l.T, l.live, &sg)) return e;
    return l.products == B_PIECES3 ? launch_strip<bert_strip_ffn_bwd_kernel<3>, BSD>(sg, l.stream, a) : launch_strip<bert_strip_ffn_bwd_kernel<0>, BSD>(sg, l.stream, a);
}
#define BFFN_BWD_CALL(c, w2T_, w1T_, woT_)                                                                                                      \
    BFfnBwdCall c;                                                                                                                              \
    c.dx2 = dx2; c.pre = pre; c.x1 = x1; c.la = la; c.w2T = w2T_; c.w1T = w1T_; c.woT = woT_; c.layer = layer; c.step_state = step_state;          \
    c.train = train; c.p_drop = p_drop; c.dz = dz; c.dpre = dpre; c.dx1 = dx1; c.dt = dt; c.d_o = d_o; c.ln_part = ln_part
extern "C" int amid_bert_strip_ffn_bwd_f32(const float* dx2, const float* pre, const float* x1, const float* const* la,
                                           const float* const* w2T, const float* const* w1T, const float* const* woT, int B, int T,
                                           const int* live, int layer, const void* step_state, int train, float p_drop, float* dz,
                                           float* dpre, float* dx1, float* dt, float* d_o, float* ln_part, void* stream) {
    BFFN_BWD_CALL(c, w2T, w1T, woT); BBWD_LAUNCH(l, B_FP32);
    return bffn_bwd(c, l);
}
// ... on bf16 pieces: w2T / w1T = the first of the four TRANSPOSED tiles' images, woT = the transposed tile's image
extern "C" int amid_bert_strip_ffn_bwd_p3_f32(const float* dx2, const float* pre, const float* x1, const float* const* la,
                                              const float* const* w2T_img, const float* const* w1T_img, const float* const* woT_img, int B, int T,
                                              const int* live, int layer, const void* step_state, int train, float p_drop, float* dz,
                                              float* dpre, float* dx1, float* dt, float* d_o, float* ln_part, void* stream) {
    BFFN_BWD_CALL(c, w2T_img, w1T_img, woT_img); BBWD_LAUNCH(l, B_PIECES3);
    return bffn_bwd(c, l);
}
#undef BFFN_BWD_CALL

// wT3: six device pointers ordered [q, k, v][domain] (transposed weights).  ffn.pre != NULL: the block below's feed-forward /
// out-projection backward (as amid_bert_strip_ffn_bwd_f32 without dx2) runs on d x in the same launch; dx is then not written.
// zero_dead (with a live list and dx): the rows of dx that belong to the sequences NOT on the list are zero-filled by extra workgroups
struct BQkvBwdCall {
    const float* dq = nullptr; const float* dk = nullptr; const float* dv = nullptr; const float* dx1 = nullptr; const float* x = nullptr;
    FamC la = nullptr, wT3 = nullptr;
    float* dx = nullptr; int zero_dead = 0; float* ln_part = nullptr;
    BFfnBwdCall ffn;
};
#define BQKV_BWD_CALL(c, wT3_, fw2T_, fw1T_, fwoT_)                                                                                             \
    BQkvBwdCall c;                                                                                                                              \
    c.dq = dq; c.dk = dk; c.dv = dv; c.dx1 = dx1; c.x = x; c.la = la; c.wT3 = wT3_; c.dx = dx; c.zero_dead = zero_dead; c.ln_part = ln_part;        \
    c.ffn.pre = fpre; c.ffn.x1 = fx1; c.ffn.la = fla; c.ffn.w2T = fw2T_; c.ffn.w1T = fw1T_; c.ffn.woT = fwoT_; c.ffn.layer = flayer;               \
    c.ffn.step_state = step_state; c.ffn.train = train; c.ffn.p_drop = p_drop; c.ffn.dz = fdz; c.ffn.dpre = fdpre; c.ffn.dx1 = fdx1;              \
    c.ffn.dt = fdt; c.ffn.d_o = fd_o; c.ffn.ln_part = fln_part

static int bqkv_bwd(const BQkvBwdCall& c, const BBwdLaunch& l) {
    AMID_CHECK_ARG(c.dq && c.dk && c.dv && c.dx1 && c.x && c.la && c.wT3 && c.ln_part);
    const bool ffn = c.ffn.pre != nullptr;
    AMID_CHECK_ARG(ffn || c.dx);
    BStripQkvBwdArgs a;
    a.dq = c.dq; a.dk = c.dk; a.dv = c.dv; a.dx1 = c.dx1; a.x = c.x; a.dx = c.dx; a.ln_part = c.ln_part;
    for (int g = 0; g < 2; ++g) {
        a.la[g] = c.la[g];
        for (int j = 0; j < 3; ++j) a.wT[j][g] = c.wT3[j * 2 + g];
    }
    BStripFfnBwdArgs f = {};
    if (ffn) if (int e = fill_bffn_bwd(f, c.ffn)) return e;
    StripGeom sg;
    if (int e = bert_strip_geom(l.B, l.T, l.live, &sg)) return e;
    a.zero_blocks = (c.zero_dead && l.live != nullptr && !ffn) ? (l.B < 256 ? l.B : 256) : 0;
    const bool p3 = l.products == B_PIECES3;
    if (ffn) return p3 ? launch_strip<bert_strip_qkv_bwd_kernel<true, 3>, BSD>(sg, l.stream, a, f)
                       : launch_strip<bert_strip_qkv_bwd_kernel<true, 0>, BSD>(sg, l.stream, a, f);
    const int grid = 2 * sg.tpg + a.zero_blocks;
    return p3 ? launch_lds<bert_strip_qkv_bwd_kernel<false, 3>>(grid, STRIP_THREADS, strip_lds_bytes<BSD>(), l.stream, a, f, sg)
              : launch_lds<bert_strip_qkv_bwd_kernel<false, 0>>(grid, STRIP_THREADS, strip_lds_bytes<BSD>(), l.stream, a, f, sg);
}
extern "C" int amid_bert_strip_qkv_bwd_f32(const float* dq, const float* dk, const float* dv, const float* dx1, const float* x,
                                           const float* const* la, const float* const* wT3, int B, int T, const int* live, float* dx,
                                           int zero_dead, float* ln_part, const float* fpre, const float* fx1, const float* const* fla,
                                           const float* const* fw2T, const float* const* fw1T, const float* const* fwoT, int flayer,
                                           const void* step_state, int train, float p_drop, float* fdz, float* fdpre, float* fdx1,
                                           float* fdt, float* fd_o, float* fln_part, void* stream) {
    BQKV_BWD_CALL(c, wT3, fw2T, fw1T, fwoT); BBWD_LAUNCH(l, B_FP32);
    return bqkv_bwd(c, l);
}
// ... on bf16 pieces: every weight argument = transposed tile images (as amid_bert_strip_ffn_bwd_p3_f32)
extern "C" int amid_bert_strip_qkv_bwd_p3_f32(const float* dq, const float* dk, const float* dv, const float* dx1, const float* x,
                                              const float* const* la, const float* const* wT3_img, int B, int T, const int* live, float* dx,
                                              int zero_dead, float* ln_part, const float* fpre, const float* fx1, const float* const* fla,
                                              const float* const* fw2T_img, const float* const* fw1T_img, const float* const* fwoT_img, int flayer,
                                              const void* step_state, int train, float p_drop, float* fdz, float* fdpre, float* fdx1,
                                              float* fdt, float* fd_o, float* fln_part, void* stream) {
    BQKV_BWD_CALL(c, wT3_img, fw2T_img, fw1T_img, fwoT_img); BBWD_LAUNCH(l, B_PIECES3);
    return bqkv_bwd(c, l);
}
#undef BQKV_BWD_CALL
#undef BBWD_LAUNCH

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
