// The arithmetic of the dense-equivalent lazy Adam (adam.hip) that more than one kernel needs: torch's single-tensor Adam step op by
// op, and the exact replay of a row's pending ZERO-gradient steps -- by the optimizer launch for the rows it updates, by the flush, by
// the catch-up launch, and, in registers only, by the gather K1 (embed.hip) for the value it hands the forward.
// Reference: torch.optim.Adam(model.parameters(), lr) over every parameter, the whole table included (train_sr.py:480, :213-215).
#pragma once
#include "common.h"
#include "rng.h"

namespace amid {

struct AdamCoef {              // per-step scalars of a REAL step, as torch computes them (double -> float at the op)
    float w1;                  // 1 - beta1                     (lerp weight)
    float beta2, w2;           // beta2, 1 - beta2
    float neg_step_size;       // -(lr / (1 - beta1^t))
    float bc2_sqrt;            // sqrt(1 - beta2^t)
    float eps;
};

// beta^s for an integer step count by repeated squaring: <= 2 log2(s) double multiplies (relative error < 1e-14, invisible after
// the coefficients are rounded to float) instead of libm's pow(double, double), several hundred fp64 instructions per call
__device__ __forceinline__ double pow_step(double b, long long s) {
    double r = 1.0;
    while (s > 0) {
        if (s & 1) r *= b;
        b *= b;
        s >>= 1;
    }
    return r;
}

__device__ __forceinline__ AdamCoef adam_coef(const StepState& st, double b1pow, double b2pow) {
    AdamCoef c;
    c.w1 = (float)(1.0 - st.beta1);
    c.beta2 = (float)st.beta2;
    c.w2 = (float)(1.0 - st.beta2);
    c.neg_step_size = (float)(-(st.lr / (1.0 - b1pow)));
    c.bc2_sqrt = (float)sqrt(1.0 - b2pow);
    c.eps = (float)st.eps;
    return c;
}
__device__ __forceinline__ AdamCoef adam_coef_now(const StepState& st) { return adam_coef(st, pow_step(st.beta1, st.step), pow_step(st.beta2, st.step)); }

// (contraction off for the step's own expressions: torch's addcmul_ / addcdiv_ are unfused, and every kernel that inlines this step must
// produce the same bits)
#pragma clang fp contract(off)
__device__ __forceinline__ void adam_elem(float& p, float& m, float& v, float g, const AdamCoef& c) {
    m = __fmaf_rn(c.w1, __fsub_rn(g, m), m);                                   // exp_avg.lerp_(grad, 1 - beta1)
    // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1-beta2): three products and a sum, each rounded -- written with the language's own
    // operators so that this file's `contract(off)` governs them (the __fmul_rn / __fadd_rn wrappers are plain `*` / `+` compiled where THEY
    // are defined, under the default contraction: inlined into two different kernels they came out as an fma in one and not in the other)
    v = (v * c.beta2) + ((c.w2 * g) * g);
    const float denom = __fadd_rn(__fdiv_rn(__fsqrt_rn(v), c.bc2_sqrt), c.eps); // (exp_avg_sq.sqrt() / bc2_sqrt).add_(eps)
    p = __fadd_rn(p, __fdiv_rn(__fmul_rn(c.neg_step_size, m), denom));          // param.addcdiv_(exp_avg, denom, value=-step_size)
}
__device__ __forceinline__ void adam_quad(float4& p, float4& m, float4& v, float4 g, const AdamCoef& c) {
    adam_elem(p.x, m.x, v.x, g.x, c);
    adam_elem(p.y, m.y, v.y, g.y, c);
    adam_elem(p.z, m.z, v.z, g.z, c);
    adam_elem(p.w, m.w, v.w, g.w, c);
}

#pragma clang fp contract(fast)

// ---- the zero-gradient step of the lazy replay ------------------------------------------------------------------------------------------
// Same recurrences for m and v (exact: one fma / one multiply); the parameter's increment through the hardware sqrt / reciprocal
// (<= 1 ulp each) instead of the IEEE divide sequences.  Its two per-step coefficients depend on the STEP NUMBER ALONE -- never on who
// replays the step, when, or from where: beta^s is the product pow_step(beta, s & ~63) * beta * ... * beta ((s & 63) factors, in this
// order), rounded bias corrections, then the hardware rcp / rsq -- so a row flushed at step t and caught up later lands on the same
// bits as one caught up in a single go (a checkpoint taken mid-run resumes bit-identically), and so do the gather's in-register replay
// and the optimizer's replay of the same row.  (Round 3 had a table of double-precision coefficients for the last 256 steps and the
// rcp / rsq form beyond it: the bits of a step depended on how old it was when it was replayed.)
struct IdleCoef { float nss, ibs; };          // -(lr rcp(1 - beta1^s)), rsq(1 - beta2^s)
struct IdleConst { float w1, beta2, eps; };
__device__ __forceinline__ IdleConst idle_const(const StepState& st) { return IdleConst{(float)(1.0 - st.beta1), (float)st.beta2, (float)st.eps}; }
constexpr int ANCHOR = 64;
struct StepPows {              // beta1^s, beta2^s of the running step s
    double b1, b2;
    __device__ __forceinline__ void at(const StepState& st, long long s) {
        const long long s0 = s & ~(long long)(ANCHOR - 1);
        b1 = pow_step(st.beta1, s0); b2 = pow_step(st.beta2, s0);
        for (long long k = s0; k < s; ++k) { b1 *= st.beta1; b2 *= st.beta2; }
    }
    // s -> s + 1
    __device__ __forceinline__ void next(const StepState& st, long long s_new) {
        if ((s_new & (ANCHOR - 1)) == 0) { b1 = pow_step(st.beta1, s_new); b2 = pow_step(st.beta2, s_new); }
        else { b1 *= st.beta1; b2 *= st.beta2; }
    }
    __device__ __forceinline__ IdleCoef coef(const StepState& st) const {
        IdleCoef c;
        c.nss = -(float)st.lr * __builtin_amdgcn_rcpf((float)(1.0 - b1));
        c.ibs = __builtin_amdgcn_rsqf((float)(1.0 - b2));
        return c;
    }
};

// coefficients of the last COEF_TAB steps (t - COEF_TAB + 1 .. t), computed once per block: a row idle for g steps replays g of them
constexpr int COEF_TAB = 256;
__device__ __forceinline__ void fill_coef_table(IdleCoef* tab, const StepState& st) {
    for (int i = threadIdx.x; i < COEF_TAB; i += blockDim.x) {
        const long long s = st.step - (COEF_TAB - 1) + i;
        if (s >= 1) { StepPows pw; pw.at(st, s); tab[i] = pw.coef(st); }
    }
    __syncthreads();
}

// K consecutive zero-gradient steps with coefficients c[0..K-1] on N elements; returns whether the LAST of them moved a parameter.  The
// moments first (two short chains), then the K denominators of an element -- independent square roots / reciprocals the hardware
// overlaps --, then the parameter's K additions in step order.
template <int N, int K>
__device__ __forceinline__ bool idle_steps(float (&p)[N], float (&m)[N], float (&v)[N], const IdleConst& k0, const IdleCoef (&c)[K]) {
    bool moved = false;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        float mk[K], rk[K];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            m[i] = __fmaf_rn(k0.w1, -m[i], m[i]);
            v[i] = __fmul_rn(v[i], k0.beta2);
            mk[k] = m[i];
            rk[k] = __builtin_amdgcn_rcpf(__fmaf_rn(__builtin_amdgcn_sqrtf(v[i]), c[k].ibs, k0.eps));
        }
        float before = p[i];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            before = p[i];
            p[i] = __fmaf_rn(__fmul_rn(c[k].nss, mk[k]), rk[k], p[i]);
        }
        moved |= p[i] != before;
    }
    return moved;
}

// Replay the zero-gradient steps s = from .. to (inclusive) on N elements of a row.  Steps older than the table take their coefficients
// from running powers (StepPows: re-anchored every 64 steps); the table holds the same values for the newest COEF_TAB steps.
// The parameter's part of a step stops mattering long before a long gap ends: the increment shrinks by ~beta1 per step (|m| does, the
// denominator and the bias corrections barely move), so once `p + increment` returns p it does so for every later step too: a lane
// whose parameters did not change in a chunk's last step skips the parameter arithmetic for the rest of the gap and only carries m and
// v on -- the SAME bits as the full replay at a fraction of its cost ("Lazy Adam over long gaps").
template <int N>
__device__ __forceinline__ void replay_elems(float (&p)[N], float (&m)[N], float (&v)[N], long long from, long long to, const StepState& st,
                                             const IdleCoef* tab) {
    constexpr int K = 4;                               // steps per chunk (the "did it move" test looks at a chunk's last step)
    const IdleConst k0 = idle_const(st);
    long long s = from;
    const long long tab_first = st.step - (COEF_TAB - 1);
    bool live = true;                                  // this lane's parameters still move
    if (s < tab_first) {
        StepPows pw;
        pw.at(st, s);
        const long long stop = (to + 1 < tab_first) ? to + 1 : tab_first;
        for (; s + K <= stop && live; s += K) {
            IdleCoef c[K];
#pragma unroll
            for (int k = 0; k < K; ++k) { c[k] = pw.coef(st); pw.next(st, s + k + 1); }
            live = idle_steps<N, K>(p, m, v, k0, c);
        }
        for (; s < stop && live; ++s) {
            const IdleCoef c[1] = {pw.coef(st)};
            live = idle_steps<N, 1>(p, m, v, k0, c);
            pw.next(st, s + 1);
        }
    }
    if (s >= tab_first) {
        for (; s + K - 1 <= to && live; s += K) {
            IdleCoef c[K];
#pragma unroll
            for (int k = 0; k < K; ++k) c[k] = tab[s + k - tab_first];
            live = idle_steps<N, K>(p, m, v, k0, c);
        }
        for (; s <= to && live; ++s) {
            const IdleCoef c[1] = {tab[s - tab_first]};
            live = idle_steps<N, 1>(p, m, v, k0, c);
        }
    }
    for (; s <= to; ++s) {
#pragma unroll
        for (int i = 0; i < N; ++i) { m[i] = __fmaf_rn(k0.w1, -m[i], m[i]); v[i] = __fmul_rn(v[i], k0.beta2); }
    }
}
__device__ __forceinline__ void replay_quad(float4& p, float4& m, float4& v, long long from, long long to, const StepState& st,
                                            const IdleCoef* tab) {
    float pp[4] = {p.x, p.y, p.z, p.w}, mm[4] = {m.x, m.y, m.z, m.w}, vv[4] = {v.x, v.y, v.z, v.w};
    replay_elems<4>(pp, mm, vv, from, to, st, tab);
    p = make_float4(pp[0], pp[1], pp[2], pp[3]); m = make_float4(mm[0], mm[1], mm[2], mm[3]); v = make_float4(vv[0], vv[1], vv[2], vv[3]);
}

// ---- the roles the optimizer kernels are built from (adam.hip, embed.hip's folded gather) ------------------------------------------------
// A row's stamp last[r] = l says: every step through l is in the row (l = 0: never touched, m = v = 0, every update is exactly 0, nothing to
// replay).  In front of the real step t a row must hold the steps through t - 1; a flush brings it through t itself.  A row stamped l owes
// the zero-gradient steps l + 1 .. end, and ends stamped `end` after a catch-up, t after the real step.
// (The role functions take plain pointers: a kernel whose own parameters are __restrict__ keeps that knowledge through the inlining, and
// one that holds its pointers in a struct -- the gradient tail -- is not given a promise it never made: with __restrict__ here its Adam
// steps were scheduled differently and cfg4's step took 0.0005 ms longer, profiles/adam_roles.md.)
__device__ __forceinline__ long long catchup_end(long long t) { return t - 1; }
__device__ __forceinline__ long long flush_end(long long t) { return t; }
// (the stamp as the caller holds it, int or long long, and both by reference: inlined, the test then compiles as it did written out at the
// call sites -- by value it cost embed.hip's folded gather 23 more exec-mask branches, profiles/adam_roles.md)
template <class Stamp>
__device__ __forceinline__ bool row_owes(const Stamp& l, const long long& end) { return l > 0 && l < end; }
template <int N>
__device__ __forceinline__ void replay_owed_elems(float (&p)[N], float (&m)[N], float (&v)[N], long long l, long long end, const StepState& st,
                                                  const IdleCoef* tab) {
    replay_elems<N>(p, m, v, l + 1, end, st, tab);
}
__device__ __forceinline__ void replay_owed_quad(float4& p, float4& m, float4& v, long long l, long long end, const StepState& st,
                                                 const IdleCoef* tab) {
    replay_quad(p, m, v, l + 1, end, st, tab);
}

// dense step of the quad at offset i / of the element at k, with the gradient g scaled by gs
__device__ __forceinline__ void dense_quad_step(float* p, float* m, float* v, long long i, float4 g, float gs,
                                                const AdamCoef& c) {
    float4 pp = ld4(p + i), mm = ld4(m + i), vv = ld4(v + i);
    adam_quad(pp, mm, vv, f4scale(g, gs), c);
    st4(p + i, pp); st4(m + i, mm); st4(v + i, vv);
}
__device__ __forceinline__ void dense_elem_step(float* p, float* m, float* v, long long k, float g, float gs,
                                                const AdamCoef& c) {
    adam_elem(p[k], m[k], v[k], g * gs, c);
}

// dense Adam over [0, n) by block `bid` of `nblocks`: a grid-stride loop over quads, the last n % 4 elements one by one.  grad.quad(i) /
// grad.one(k): the gradient at quad i / element k (FlatGrad: read from a flat buffer; the gathered optimizer's: summed over the ranks)
struct FlatGrad {
    const float* __restrict__ g;
    __device__ __forceinline__ float4 quad(long long i) const { return ld4(g + i); }
    __device__ __forceinline__ float one(long long k) const { return g[k]; }
};
template <class Grad>
__device__ __forceinline__ void dense_adam_range(float* p, float* m, float* v, long long n, long long bid,
                                                 long long nblocks, const Grad& grad, float gs, const AdamCoef& c) {
    const long long stride = nblocks * blockDim.x * 4;
    for (long long i = (bid * blockDim.x + threadIdx.x) * 4; i < n; i += stride) {
        if (i + 4 <= n) dense_quad_step(p, m, v, i, grad.quad(i), gs, c);
        else for (long long k = i; k < n; ++k) dense_elem_step(p, m, v, k, grad.one(k), gs, c);
    }
}

// the real step t = st.step of a row's quad already in registers: what the row owes (lag = row_owes(l, catchup_end(t))), then the step
__device__ __forceinline__ void row_quad_step(float4& p, float4& m, float4& v, float4 g, float gs, long long l, bool lag, const StepState& st,
                                              const IdleCoef* tab, const AdamCoef& cnow) {
    if (lag) replay_owed_quad(p, m, v, l, catchup_end(st.step), st, tab);
    adam_quad(p, m, v, f4scale(g, gs), cnow);
}

// A half-wave (sub = its lane, 0 .. 31) on row r, a quad per lane and round.  grad(c): the gradient of column quad c, called AFTER the loads
// of the row's parameter and moments are issued, so that they are in flight under whatever it does.
//   ROW_STEP     what the row owes, then the real step t with grad(c); stamp t
//   ROW_CATCHUP  what the row owes in front of step t, nothing for a row that owes nothing; stamp t - 1
//   ROW_FLUSH    the same through step t; stamp t
//   ROW_SHIP     nothing is applied: grad(c) alone runs (it stores what it sums)
enum RowMode { ROW_STEP, ROW_CATCHUP, ROW_FLUSH, ROW_SHIP };
struct NoGrad { __device__ __forceinline__ float4 operator()(int) const { return make_float4(0.f, 0.f, 0.f, 0.f); } };
template <RowMode MODE, class Grad = NoGrad>
__device__ __forceinline__ void halfwave_row(float* table, float* m_tab, float* v_tab, int* last,
                                             long long r, int D, int sub, const StepState& st, const IdleCoef* tab, const AdamCoef& cnow = AdamCoef{},
                                             float gs = 1.0f, const Grad& grad = Grad{}) {
    if constexpr (MODE == ROW_SHIP) {
        for (int c = sub; c < (D >> 2); c += 32) grad(c);
    } else {
        const long long t = st.step, end = MODE == ROW_FLUSH ? flush_end(t) : catchup_end(t);
        const long long l = last[r];
        const bool lag = row_owes(l, end);
        if (MODE != ROW_STEP && !lag) return;
        for (int c = sub; c < (D >> 2); c += 32) {
            const long long off = r * D + 4 * c;
            float4 p = ld4(table + off), m = ld4(m_tab + off), v = ld4(v_tab + off);
            if constexpr (MODE == ROW_STEP) row_quad_step(p, m, v, grad(c), gs, l, lag, st, tab, cnow);
            else replay_owed_quad(p, m, v, l, end, st, tab);
            st4(table + off, p); st4(m_tab + off, m); st4(v_tab + off, v);
        }
        __builtin_amdgcn_wave_barrier();
        if (sub == 0) last[r] = MODE == ROW_STEP ? (int)t : (int)end;
    }
}

// A wave (lane = 0 .. 63) replays what row r, stamped l, owes in front of step t = st.step: two elements per lane -- a replay is a chain of
// dependent steps bound by the quarter-rate sqrt / rcp, the fewer elements a lane carries the shorter the chain.  The caller stamps the row.
// NT: non-temporal loads, for a launch in which a lagging row is read once per step and the tables are far larger than the caches (the
// stress's catch-up launch 140.5 -> 136.7 us)
template <bool NT>
__device__ __forceinline__ void wave_replay_row(float* table, float* m_tab, float* v_tab, long long r, long long l, int D, int lane,
                                                const StepState& st, const IdleCoef* tab) {
    typedef float f2 __attribute__((ext_vector_type(2)));
    for (int c = lane; c < (D >> 1); c += 64) {
        const long long off = r * D + 2 * c;
        f2 pn, mn, vn;
        if constexpr (NT) {
            pn = __builtin_nontemporal_load((const f2*)(table + off)); mn = __builtin_nontemporal_load((const f2*)(m_tab + off));
            vn = __builtin_nontemporal_load((const f2*)(v_tab + off));
        } else {
            pn = *(const f2*)(table + off); mn = *(const f2*)(m_tab + off); vn = *(const f2*)(v_tab + off);
        }
        float p[2] = {pn[0], pn[1]}, m[2] = {mn[0], mn[1]}, v[2] = {vn[0], vn[1]};
        replay_owed_elems<2>(p, m, v, l, catchup_end(st.step), st, tab);
        *reinterpret_cast<float2*>(table + off) = make_float2(p[0], p[1]);
        *reinterpret_cast<float2*>(m_tab + off) = make_float2(m[0], m[1]);
        *reinterpret_cast<float2*>(v_tab + off) = make_float2(v[0], v[1]);
    }
}

}  // namespace amid
