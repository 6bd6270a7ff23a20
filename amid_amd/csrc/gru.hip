// GRU4Rec's encoder (reference: GRU4Rec model_seq.py:56-113 -- one nn.GRU(D, D, 1, batch_first=True) per domain, h0 = 0, every one of
// the T positions stepped through, pads included; autograd of the same): the input projection, the recurrence forward (saving and
// inference forms), the recurrence backward and the data gradient.  D = 128 only.
//
// Tiling.  A workgroup of 8 waves takes 16 sequences of ONE domain (a tile never straddles the two halves of a live list).  Every product
// here is [16 sequences, K] x [K, N] on v_mfma_f32_16x16x4_f32 with the sequence as the M index, so a sequence's result is a function of
// its own operand row only: the same bits in any tile and any slot, with or without a live list.  Wave w owns 16 output columns and keeps
// its slice of the weight matrix in registers for the whole launch, 96 per lane:
//   forward  (proj, rec_fwd):  K = 128, columns 16 w .. 16 w + 15 of all three gates   (32 k-steps x 3 gates)
//   backward (rec_bwd, dx):    K = 384, columns 16 w .. 16 w + 15 of the D outputs       (96 k-steps)
// Lane (i = lane & 15, gq = lane >> 4) feeds k-slot gq of every MFMA; slot gq walks the CONTIGUOUS k range [gq K/4, (gq + 1) K/4) so that the
// A operand comes out of LDS as float4 reads.  The accumulators hold rows 4 gq + r (r < 4) of column 16 w + i: the gate arithmetic of
// a (sequence, column) pair stays in one lane from step 0 to step T - 1, its previous hidden value in a register.
// The recurrence exchanges h_t (forward, 8 KB) / dGh_t (backward, 24 KB) through double-buffered LDS: one barrier a step.
#include "common.h"
#include "amid_hip.h"

namespace amid {

constexpr int GD = 128, G3 = 3 * GD;
constexpr int GRU_THREADS = 512, GRU_SEQ = 16;
constexpr int LDH = GD + 4, LDG = G3 + 4;          // LDS row strides (floats)
constexpr int GRU_TC = 4;                          // time steps per workgroup of the row products (proj, dx)

__device__ __forceinline__ f32x4 gmfma(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
__device__ __forceinline__ float gsigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }

// The tile of this workgroup: domain g, sequences seq[0 .. n) (batch rows), or n = 0 (nothing to do).  Without a list: 2 ceil(B / 16)
// workgroups, domain-major.  With one: ceil(B / 16) + 1 workgroups (the host does not know n0); domain 0's tiles first.
struct GruTile { int g, n; };
__device__ __forceinline__ GruTile gru_tile(const int* __restrict__ live, int B, int* __restrict__ seq /* LDS [16] */) {
    GruTile t;
    int s0, s1;
    if (live) {
        const int n0 = min(max(live[B], 0), B);
        const int nt0 = (n0 + GRU_SEQ - 1) / GRU_SEQ;
        const int k = blockIdx.x;
        if (k < nt0) { t.g = 0; s0 = k * GRU_SEQ; s1 = min(n0, s0 + GRU_SEQ); }
        else { t.g = 1; s0 = n0 + (k - nt0) * GRU_SEQ; s1 = min(B, s0 + GRU_SEQ); }
    } else {
        const int ntb = (B + GRU_SEQ - 1) / GRU_SEQ;
        t.g = blockIdx.x / ntb;
        s0 = (blockIdx.x % ntb) * GRU_SEQ; s1 = min(B, s0 + GRU_SEQ);
    }
    t.n = max(0, s1 - s0);
    if (threadIdx.x < GRU_SEQ) {
        int b = -1;
        if ((int)threadIdx.x < t.n) b = live ? min(max(live[s0 + threadIdx.x], 0), B - 1) : s0 + (int)threadIdx.x;
        seq[threadIdx.x] = b;
    }
    return t;
}

// B fragments of out = A W^T, W [3 D, D] row-major: wf[q][s] = W[q D + 16 w + i][32 gq + s]
__device__ __forceinline__ void load_w_fwd(const float* __restrict__ W, int w, int i, int gq, float (&wf)[3][32]) {
#pragma unroll
    for (int q = 0; q < 3; ++q)
#pragma unroll
        for (int s4 = 0; s4 < 8; ++s4) {
            const float4 v = ld4(W + (size_t)(q * GD + 16 * w + i) * GD + 32 * gq + 4 * s4);
            wf[q][4 * s4] = v.x; wf[q][4 * s4 + 1] = v.y; wf[q][4 * s4 + 2] = v.z; wf[q][4 * s4 + 3] = v.w;
        }
}
// B fragments of out = A W, W [3 D, D] row-major: wb[s] = W[96 gq + s][16 w + i]
__device__ __forceinline__ void load_w_bwd(const float* __restrict__ W, int w, int i, int gq, float (&wb)[96]) {
#pragma unroll
    for (int s = 0; s < 96; ++s) wb[s] = W[(size_t)(96 * gq + s) * GD + 16 * w + i];
}
// acc[q] += A[16, 128] (LDS, stride LDH) x wf[q]
__device__ __forceinline__ void prod_fwd(const float* __restrict__ As, int i, int gq, const float (&wf)[3][32], f32x4 (&acc)[3]) {
#pragma unroll
    for (int s4 = 0; s4 < 8; ++s4) {
        const float4 a = ld4(As + i * LDH + 32 * gq + 4 * s4);
#pragma unroll
        for (int q = 0; q < 3; ++q) acc[q] = gmfma(a.x, wf[q][4 * s4], acc[q]);
#pragma unroll
        for (int q = 0; q < 3; ++q) acc[q] = gmfma(a.y, wf[q][4 * s4 + 1], acc[q]);
#pragma unroll
        for (int q = 0; q < 3; ++q) acc[q] = gmfma(a.z, wf[q][4 * s4 + 2], acc[q]);
#pragma unroll
        for (int q = 0; q < 3; ++q) acc[q] = gmfma(a.w, wf[q][4 * s4 + 3], acc[q]);
    }
}
// A[16, 384] (LDS, stride LDG) x wb -> [16, 16]: three accumulator chains (one per 32 k-steps of every slot), summed in a fixed order
__device__ __forceinline__ f32x4 prod_bwd(const float* __restrict__ As, int i, int gq, const float (&wb)[96]) {
    f32x4 acc[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) acc[c] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s4 = 0; s4 < 8; ++s4) {
        float4 a[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) a[c] = ld4(As + i * LDG + 96 * gq + 32 * c + 4 * s4);
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[c] = gmfma(a[c].x, wb[32 * c + 4 * s4], acc[c]);
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[c] = gmfma(a[c].y, wb[32 * c + 4 * s4 + 1], acc[c]);
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[c] = gmfma(a[c].z, wb[32 * c + 4 * s4 + 2], acc[c]);
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[c] = gmfma(a[c].w, wb[32 * c + 4 * s4 + 3], acc[c]);
    }
    return (acc[0] + acc[1]) + acc[2];
}

struct GruProjArgs { const float* x; const float* w[2]; const float* b[2]; float* gi; const int* live; int B, T; };

// Gi[row] = X[row] W_ih^T + b_ih for the rows of the tile's sequences at the GRU_TC steps of blockIdx.y
__global__ __launch_bounds__(GRU_THREADS) void gru_proj_kernel(const GruProjArgs a) {
    __shared__ __attribute__((aligned(16))) float xs[GRU_SEQ * LDH];
    __shared__ int seq[GRU_SEQ];
    const GruTile tl = gru_tile(a.live, a.B, seq);
    if (tl.n == 0) return;
    const int w = wave_id(), lane = lane_id(), i = lane & 15, gq = lane >> 4;
    float wf[3][32];
    load_w_fwd(a.w[tl.g], w, i, gq, wf);
    float bias[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) bias[q] = a.b[tl.g][q * GD + 16 * w + i];
    __syncthreads();
    const int t0 = blockIdx.y * GRU_TC, t1 = min(a.T, t0 + GRU_TC);
    const int lm = threadIdx.x >> 5, lc = (threadIdx.x & 31) * 4;          // staging: thread -> (sequence, 4 columns)
    for (int t = t0; t < t1; ++t) {
        const int sb = seq[lm];
        const float4 v = sb >= 0 ? ld4(a.x + ((size_t)(tl.g * a.B + sb) * a.T + t) * GD + lc) : make_float4(0.f, 0.f, 0.f, 0.f);
        __syncthreads();                       // (the previous step's reads are done)
        st4(xs + lm * LDH + lc, v);
        __syncthreads();
        f32x4 acc[3];
#pragma unroll
        for (int q = 0; q < 3; ++q) acc[q] = f32x4{bias[q], bias[q], bias[q], bias[q]};
        prod_fwd(xs, i, gq, wf, acc);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int sq = seq[4 * gq + r];
            if (sq < 0) continue;
            float* o = a.gi + ((size_t)(tl.g * a.B + sq) * a.T + t) * G3 + 16 * w + i;
#pragma unroll
            for (int q = 0; q < 3; ++q) o[q * GD] = acc[q][r];
        }
    }
}

struct GruFwdArgs { const float* gi; const float* w[2]; const float* b[2]; float* h; float* gates; float* ghn; float* hprev; const int* live; int B, T; };

// One recurrence step's arithmetic lives in this kernel only: the saving and the inference form are its two instantiations.
template <bool SAVE>
__global__ __launch_bounds__(GRU_THREADS) void gru_rec_fwd_kernel(const GruFwdArgs a) {
    __shared__ __attribute__((aligned(16))) float hs[2][GRU_SEQ * LDH];
    __shared__ int seq[GRU_SEQ];
    const GruTile tl = gru_tile(a.live, a.B, seq);
    if (tl.n == 0) return;
    const int w = wave_id(), lane = lane_id(), i = lane & 15, gq = lane >> 4;
    const int col = 16 * w + i;
    float wf[3][32];
    load_w_fwd(a.w[tl.g], w, i, gq, wf);
    float bias[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) bias[q] = a.b[tl.g][q * GD + col];
    for (int k = threadIdx.x; k < GRU_SEQ * LDH; k += GRU_THREADS) hs[0][k] = 0.f;
    __syncthreads();
    const int T = a.T;
    size_t row0[4];
    bool ok[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int sq = seq[4 * gq + r];
        ok[r] = sq >= 0;
        row0[r] = (size_t)(tl.g * a.B + max(sq, 0)) * T;
    }
    float hp[4] = {0.f, 0.f, 0.f, 0.f};
    float gin[3][4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int q = 0; q < 3; ++q) gin[q][r] = ok[r] ? a.gi[row0[r] * G3 + q * GD + col] : 0.f;
    for (int t = 0; t < T; ++t) {
        const int cur = t & 1;
        float gic[3][4];
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int q = 0; q < 3; ++q) gic[q][r] = gin[q][r];
        if (t + 1 < T) {                       // the next step's input gates: their loads fly under this step's products
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int q = 0; q < 3; ++q) gin[q][r] = ok[r] ? a.gi[(row0[r] + t + 1) * G3 + q * GD + col] : 0.f;
        }
        f32x4 acc[3];
#pragma unroll
        for (int q = 0; q < 3; ++q) acc[q] = f32x4{bias[q], bias[q], bias[q], bias[q]};
        prod_fwd(hs[cur], i, gq, wf, acc);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float rg = gsigmoid(gic[0][r] + acc[0][r]);
            const float zg = gsigmoid(gic[1][r] + acc[1][r]);
            const float ng = tanhf(gic[2][r] + rg * acc[2][r]);
            const float hn = (1.0f - zg) * ng + zg * hp[r];
            if (ok[r]) {
                const size_t row = row0[r] + t;
                if (SAVE) {
                    a.gates[row * G3 + col] = rg;
                    a.gates[row * G3 + GD + col] = zg;
                    a.gates[row * G3 + 2 * GD + col] = ng;
                    a.ghn[row * GD + col] = acc[2][r];
                    a.hprev[row * GD + col] = hp[r];
                }
                a.h[row * GD + col] = hn;
            }
            hs[cur ^ 1][(4 * gq + r) * LDH + col] = hn;
            hp[r] = hn;
        }
        __syncthreads();
    }
}

struct GruBwdArgs { const float* dh; const float* gates; const float* ghn; const float* hprev; const float* w[2]; float* dgi; float* dgh;
                    const int* live; int B, T, zero_dead; };

// zero the rows [t0, t1) of the tile's sequences in the OTHER domain (n_col floats a row, a multiple of 4)
__device__ __forceinline__ void zero_other_domain(float* __restrict__ out, int n_col, const int* seq, int n, int g, int B, int T, int t0, int t1) {
    const int c4 = n_col / 4, per = (t1 - t0) * c4;
    for (int m = 0; m < n; ++m) {
        float* p = out + ((size_t)((1 - g) * B + seq[m]) * T + t0) * n_col;
        for (int k = threadIdx.x; k < per; k += GRU_THREADS) st4(p + 4 * (size_t)k, make_float4(0.f, 0.f, 0.f, 0.f));
    }
}

__global__ __launch_bounds__(GRU_THREADS) void gru_rec_bwd_kernel(const GruBwdArgs a) {
    __shared__ __attribute__((aligned(16))) float gs[2][GRU_SEQ * LDG];
    __shared__ int seq[GRU_SEQ];
    const GruTile tl = gru_tile(a.live, a.B, seq);
    if (tl.n == 0) return;
    const int w = wave_id(), lane = lane_id(), i = lane & 15, gq = lane >> 4;
    const int col = 16 * w + i;
    float wb[96];
    load_w_bwd(a.w[tl.g], w, i, gq, wb);
    __syncthreads();
    const int T = a.T;
    if (a.live && a.zero_dead) {
        zero_other_domain(a.dgi, G3, seq, tl.n, tl.g, a.B, T, 0, T);
        zero_other_domain(a.dgh, G3, seq, tl.n, tl.g, a.B, T, 0, T);
    }
    size_t row0[4];
    bool ok[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int sq = seq[4 * gq + r];
        ok[r] = sq >= 0;
        row0[r] = (size_t)(tl.g * a.B + max(sq, 0)) * T;
    }
    float carry[4] = {0.f, 0.f, 0.f, 0.f};
    // what a step reads from HBM -- the saved gates, ghn, hprev and the cotangent -- does not depend on the carry: step t - 1's values are
    // loaded under step t's product
    float nx[6][4];
    auto fetch = [&](int t) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const size_t row = row0[r] + t;
#pragma unroll
            for (int q = 0; q < 3; ++q) nx[q][r] = ok[r] ? a.gates[row * G3 + q * GD + col] : 0.f;
            nx[3][r] = ok[r] ? a.ghn[row * GD + col] : 0.f;
            nx[4][r] = ok[r] ? a.hprev[row * GD + col] : 0.f;
            nx[5][r] = ok[r] ? a.dh[row * GD + col] : 0.f;
        }
    };
    fetch(T - 1);
    for (int t = T - 1; t >= 0; --t) {
        const int cur = t & 1;
        float sv[6][4];
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int q = 0; q < 6; ++q) sv[q][r] = nx[q][r];
        if (t > 0) fetch(t - 1);
        float keep[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float rg = sv[0][r], zg = sv[1][r], ng = sv[2][r], gh = sv[3][r], hp = sv[4][r];
            const float dh = sv[5][r] + carry[r];
            const float dnp = dh * (1.0f - zg) * (1.0f - ng * ng);
            const float dzp = dh * (hp - ng) * zg * (1.0f - zg);
            const float drp = dnp * gh * rg * (1.0f - rg);
            const float dgn = dnp * rg;
            keep[r] = dh * zg;
            if (ok[r]) {
                const size_t row = row0[r] + t;
                a.dgi[row * G3 + col] = drp; a.dgi[row * G3 + GD + col] = dzp; a.dgi[row * G3 + 2 * GD + col] = dnp;
                a.dgh[row * G3 + col] = drp; a.dgh[row * G3 + GD + col] = dzp; a.dgh[row * G3 + 2 * GD + col] = dgn;
            }
            float* g = gs[cur] + (4 * gq + r) * LDG + col;      // (an empty slot: zeros in, zeros out -- its carry stays zero)
            g[0] = drp; g[GD] = dzp; g[2 * GD] = dgn;
        }
        if (t == 0) break;                     // (no step in front of the first one takes a carry)
        __syncthreads();
        const f32x4 p = prod_bwd(gs[cur], i, gq, wb);
#pragma unroll
        for (int r = 0; r < 4; ++r) carry[r] = keep[r] + p[r];
    }
}

struct GruDxArgs { const float* dgi; const float* w[2]; float* dx; const int* live; int B, T, zero_dead; };

// dX[row] = dGi[row] W_ih for the rows of the tile's sequences at the GRU_TC steps of blockIdx.y
__global__ __launch_bounds__(GRU_THREADS) void gru_dx_kernel(const GruDxArgs a) {
    __shared__ __attribute__((aligned(16))) float gs[GRU_SEQ * LDG];
    __shared__ int seq[GRU_SEQ];
    const GruTile tl = gru_tile(a.live, a.B, seq);
    if (tl.n == 0) return;
    const int w = wave_id(), lane = lane_id(), i = lane & 15, gq = lane >> 4;
    float wb[96];
    load_w_bwd(a.w[tl.g], w, i, gq, wb);
    __syncthreads();
    const int t0 = blockIdx.y * GRU_TC, t1 = min(a.T, t0 + GRU_TC);
    if (a.live && a.zero_dead) zero_other_domain(a.dx, GD, seq, tl.n, tl.g, a.B, a.T, t0, t1);
    for (int t = t0; t < t1; ++t) {
        __syncthreads();                       // (the previous step's reads are done)
        for (int k = threadIdx.x; k < GRU_SEQ * (G3 / 4); k += GRU_THREADS) {
            const int m = k / (G3 / 4), c = (k % (G3 / 4)) * 4;
            const int sb = seq[m];
            st4(gs + m * LDG + c, sb >= 0 ? ld4(a.dgi + ((size_t)(tl.g * a.B + sb) * a.T + t) * G3 + c) : make_float4(0.f, 0.f, 0.f, 0.f));
        }
        __syncthreads();
        const f32x4 p = prod_bwd(gs, i, gq, wb);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int sq = seq[4 * gq + r];
            if (sq >= 0) a.dx[((size_t)(tl.g * a.B + sq) * a.T + t) * GD + 16 * w + i] = p[r];
        }
    }
}

}  // namespace amid

using namespace amid;

extern "C" int amid_gru_supported(int B, int T, int D) {
    return (D == GD && B > 0 && T > 0 && 2LL * B * T * G3 * 4 <= 0x7FFFFFF0LL) ? 1 : 0;
}

static int gru_shape(int B, int T, int D) {
    if (B <= 0 || T <= 0 || D <= 0) return AMID_ERR_ARG;
    return amid_gru_supported(B, T, D) ? AMID_OK : AMID_ERR_UNSUPPORTED;
}
static unsigned gru_tiles(int B, const int* live) {
    const int ntb = (B + GRU_SEQ - 1) / GRU_SEQ;
    return (unsigned)(live ? ntb + 1 : 2 * ntb);
}

extern "C" int amid_gru_proj_fwd_f32(const float* x, const float* const* w_ih, const float* const* b_ih, int B, int T, int D, const int* live,
                                     float* gi, void* stream) {
    AMID_CHECK_ARG(x && w_ih && b_ih && gi);
    if (int e = gru_shape(B, T, D)) return e;
    AMID_CHECK_ARG(w_ih[0] && w_ih[1] && b_ih[0] && b_ih[1]);
    GruProjArgs a{x, {w_ih[0], w_ih[1]}, {b_ih[0], b_ih[1]}, gi, live, B, T};
    gru_proj_kernel<<<dim3(gru_tiles(B, live), (T + GRU_TC - 1) / GRU_TC), GRU_THREADS, 0, (hipStream_t)stream>>>(a);
    AMID_LAUNCH_CHECK();
    return AMID_OK;
}

extern "C" int amid_gru_rec_fwd_f32(const float* gi, const float* const* w_hh, const float* const* b_hh, int B, int T, int D, const int* live,
                                    float* h, float* gates, float* ghn, float* hprev, void* stream) {
    AMID_CHECK_ARG(gi && w_hh && b_hh && h && gates && ghn && hprev);
    if (int e = gru_shape(B, T, D)) return e;
    AMID_CHECK_ARG(w_hh[0] && w_hh[1] && b_hh[0] && b_hh[1]);
    GruFwdArgs a{gi, {w_hh[0], w_hh[1]}, {b_hh[0], b_hh[1]}, h, gates, ghn, hprev, live, B, T};
    gru_rec_fwd_kernel<true><<<gru_tiles(B, live), GRU_THREADS, 0, (hipStream_t)stream>>>(a);
    AMID_LAUNCH_CHECK();
    return AMID_OK;
}

extern "C" int amid_gru_rec_fwd_infer_f32(const float* gi, const float* const* w_hh, const float* const* b_hh, int B, int T, int D,
                                          const int* live, float* h, void* stream) {
    AMID_CHECK_ARG(gi && w_hh && b_hh && h);
    if (int e = gru_shape(B, T, D)) return e;
    AMID_CHECK_ARG(w_hh[0] && w_hh[1] && b_hh[0] && b_hh[1]);
    GruFwdArgs a{gi, {w_hh[0], w_hh[1]}, {b_hh[0], b_hh[1]}, h, nullptr, nullptr, nullptr, live, B, T};
    gru_rec_fwd_kernel<false><<<gru_tiles(B, live), GRU_THREADS, 0, (hipStream_t)stream>>>(a);
    AMID_LAUNCH_CHECK();
    return AMID_OK;
}

extern "C" int amid_gru_rec_bwd_f32(const float* dh, const float* gates, const float* ghn, const float* hprev, const float* const* w_hh, int B,
                                    int T, int D, const int* live, int zero_dead, float* dgi, float* dgh, void* stream) {
    AMID_CHECK_ARG(dh && gates && ghn && hprev && w_hh && dgi && dgh);
    if (int e = gru_shape(B, T, D)) return e;
    AMID_CHECK_ARG(w_hh[0] && w_hh[1]);
    GruBwdArgs a{dh, gates, ghn, hprev, {w_hh[0], w_hh[1]}, dgi, dgh, live, B, T, zero_dead};
    gru_rec_bwd_kernel<<<gru_tiles(B, live), GRU_THREADS, 0, (hipStream_t)stream>>>(a);
    AMID_LAUNCH_CHECK();
    return AMID_OK;
}

extern "C" int amid_gru_dx_f32(const float* dgi, const float* const* w_ih, int B, int T, int D, const int* live, int zero_dead, float* dx,
                               void* stream) {
    AMID_CHECK_ARG(dgi && w_ih && dx);
    if (int e = gru_shape(B, T, D)) return e;
    AMID_CHECK_ARG(w_ih[0] && w_ih[1]);
    GruDxArgs a{dgi, {w_ih[0], w_ih[1]}, dx, live, B, T, zero_dead};
    gru_dx_kernel<<<dim3(gru_tiles(B, live), (T + GRU_TC - 1) / GRU_TC), GRU_THREADS, 0, (hipStream_t)stream>>>(a);
    AMID_LAUNCH_CHECK();
    return AMID_OK;
}
