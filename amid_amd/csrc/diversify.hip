// Diversified top-K: greedy Maximal Marginal Relevance (MMR) over each row's OWN list.  Row b owns cand[cand_off[b] .. cand_off[b + 1]),
// int64 ids of table [n_rows, D] rows with a relevance rel (fp32) per entry; lists are ragged, empty lists and duplicates allowed.
//
// The operation (metric 0 = dot, 1 = cosine; lambda in [0, 1]; 1 <= K <= M <= 256, M = the shortlist):
//   1. An entry is ABSENT if its id lies outside [0, n_rows) or its rel is NaN.  An id outside the table also raises AMID_FLAG_INDEX_RANGE
//      and is never dereferenced.  (NaN is what rank_lists.hip writes into list_scores for such ids, so the two compose.)
//   2. The SHORTLIST holds the M best present entries under rank_lists.hip's total order: larger rel first, ties to the lower id, further
//      ties to the lower position (ragged_lists.h's list, so neither the shortlist nor its order depends on how a long list is cut into
//      tiles and units).  Duplicates may occupy shortlist slots.
//   3. Pick 1 is the head of the shortlist: value = lambda * rel, max_sim = 0.
//   4. Pick j >= 2 looks at the shortlist entries that are not picked yet and whose id differs from every picked id.  For each,
//      m(c) = max over the picked s of sim(c, s), a running fmaxf in pick order, and
//          v(c) = (lambda * rel(c)) - ((1 - lambda) * m(c))
//      with contraction off, 1 - lambda formed once in fp32: two multiplications and one subtraction, in that order.  The largest v is
//      picked; ties go to the lower id, then to the lower position.  (An entry whose v is NaN is never picked.)  It stops when K are
//      picked or nothing remains.
//   5. sim(c, s) is neighbors.hip's score of candidate row s for query row c under the same metric, bit for bit (sim_parts.h): the dot
//      product is the fmaf chain over elements e, D/4 + e, 2 D/4 + e, 3 D/4 + e for e = 0 .. D/4 - 1 from 0; cosine is
//      (dot * inv(c)) * inv(s) with inv(row) = 1 / max(|row|, 1e-8) formed as nb_norm_kernel forms it.
//   6. Outputs [B, K]: ids, rel (the picked entries' relevance), value (v at the pick), max_sim (m at the pick), positions (index inside
//      the row's own list); padding -1 / -inf / -inf / -inf / -1.
// So with lambda = 1 the result is the shortlist order with ids deduplicated; the first pick depends on neither lambda nor metric; and a
// row's picks depend on nothing but its own list.
//
// Launches (all on the caller's stream, no host synchronisation, no host read of an offset):
//   mm_prefix_kernel  one workgroup: the exclusive prefix unit_pre [B + 1] of the rows' unit counts (ragged_lists.h)
//   mm_short_kernel   persistent workgroups over the units: a thread an entry of a tile offers (rel, (id << 32) | position) to the unit's
//                     running best-M list -> part_s / part_k [units][M]
//   mm_pick_kernel    persistent workgroups over the rows, a thread a shortlist entry.  The row's units' lists through the same merge ->
//                     the shortlist in LDS.  Thread t keeps entry t's table row in REGISTERS (D floats, gathered once; M <= 256 = the
//                     workgroup) with its rel, key, inverse norm and running m.  A round: the picked thread puts its row, inverse norm and
//                     id into LDS; every live thread walks the fmaf chain of its own row against that row (broadcast 16-byte LDS reads),
//                     updates m and v; the arg-max under the tie rule goes through DPP inside a wave and four LDS slots across the waves
//                     (double-buffered by the round's parity): two barriers a round, K rounds.  Nothing of an M x M matrix exists
//                     anywhere: M (M - 1) / 2 similarities at most are formed, each once, in registers.
#include "ragged_lists.h"
#include "sim_parts.h"

namespace amid {

#pragma clang fp contract(off)

struct MmArgs {
    const long long* cand; const long long* cand_off; const float* rel; long long n_cand;
    const float* table; long long n_rows;
    int B, D, metric, K, M;
    float lambda;
    int per;                                    // tiles per unit
    int unit_bound;                             // rows of part_s / part_k: the prefix never counts more units than this
    int* flags;
    int* unit_pre;                              // workspace [B + 1]
    float* part_s; unsigned long long* part_k;  // workspace [units][M]
    long long* out_ids; float* out_rel; float* out_value; float* out_max_sim; long long* out_pos;      // [B][K]; all but out_ids may be null
};

__global__ __launch_bounds__(FR_THREADS) void mm_prefix_kernel(const MmArgs a) {
    rl_unit_prefix(a.cand_off, a.n_cand, a.B, a.per, a.unit_bound, a.unit_pre, a.flags);
}

// ---- a unit's tiles -> its best-M list ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(FR_THREADS) void mm_short_kernel(const MmArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char sm_raw[];
    const int M = a.M, tid = threadIdx.x;
    const RlLds c = rl_carve(sm_raw, M);
    const int n_units = a.unit_pre[a.B];
    for (int unit = blockIdx.x; unit < n_units; unit += gridDim.x) {
        const int b = rl_row_of_unit(a.unit_pre, a.B, unit);           // (uniform)
        long long lo, len;
        rl_clamp_list(a.cand_off, a.n_cand, b, lo, len, nullptr);
        const long long n_tiles = (len + RL_TILE - 1) / RL_TILE;
        const long long t0 = (long long)(unit - a.unit_pre[b]) * a.per, t1 = min(n_tiles, t0 + a.per);
        rl_list_reset(c);                                              // (the previous unit's list is written out)
        for (long long t = t0; t < t1; ++t) {
            const long long p = t * RL_TILE + tid;
            const bool on = p < len;
            const long long id = on ? a.cand[lo + p] : -1;
            const float r = on ? a.rel[lo + p] : 0.f;
            const bool in = id >= 0 && id < a.n_rows;
            if (on && !in) atomicOr(a.flags, AMID_FLAG_INDEX_RANGE);
            rl_offer(c, M, on && in && r == r, r, ((unsigned long long)id << 32) | (unsigned long long)p);
        }
        rl_list_close(c, M);
        const long long o = (long long)unit * M;
        for (int k = tid; k < M; k += FR_THREADS) { a.part_s[o + k] = c.L.s[k]; a.part_k[o + k] = c.L.key[k]; }
    }
}

// ---- the arg-max of a round -------------------------------------------------------------------------------------------------------------------------
template <int CTRL>
__device__ __forceinline__ void mm_best_step(float& v, unsigned long long& k) {
    const float ov = dpp_move<CTRL>(v);
    const unsigned lo = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)k, CTRL, 0xF, 0xF, true);
    const unsigned hi = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)(k >> 32), CTRL, 0xF, 0xF, true);
    const unsigned long long ok = ((unsigned long long)hi << 32) | lo;
    if (rl_before(ov, ok, v, k)) { v = ov; k = ok; }
}
__device__ __forceinline__ unsigned long long mm_lane_key(unsigned long long k, int lane) {
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)k, lane);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(k >> 32), lane);
    return ((unsigned long long)hi << 32) | lo;
}
// the best (v, key) of the wave under rl_before, in every lane (every lane of the wave calls this; keys are unique or RL_KEY_NONE, so the
// order is total and every lane arrives at the same entry: group_allreduce's exchanges with a compound operand)
__device__ __forceinline__ void mm_wave_best(float& v, unsigned long long& k) {
    mm_best_step<0xB1>(v, k);
    mm_best_step<0x4E>(v, k);
    mm_best_step<0x141>(v, k);
    mm_best_step<0x140>(v, k);
    float bv = lane_value(v, 0);
    unsigned long long bk = mm_lane_key(k, 0);
#pragma unroll
    for (int r = 16; r < kWave; r += 16) {
        const float ov = lane_value(v, r);
        const unsigned long long ok = mm_lane_key(k, r);
        if (rl_before(ov, ok, bv, bk)) { bv = ov; bk = ok; }
    }
    v = bv; k = bk;
}

// ---- a row: its units' lists -> the shortlist -> K greedy picks ---------------------------------------------------------------------------------------
// LDS: the list's (rl_list_lds_bytes(M)) | the picked row [D] | inverse norms [FR_THREADS] | wave bests: keys [2][4] (8-byte), values [2][4] |
// the picked entry's id (8-byte), its inverse norm, 1 spare
__host__ __device__ inline size_t mm_pick_lds_bytes(int D, int M) { return rl_list_lds_bytes(M) + (size_t)4 * (D + FR_THREADS) + 8 * 8 + 4 * 8 + 16; }

template <int D>
__global__ __launch_bounds__(FR_THREADS) void mm_pick_kernel(const MmArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char sm_raw[];
    constexpr int DQ = D / 4, NW = FR_THREADS / kWave;
    const int M = a.M, K = a.K, tid = threadIdx.x, part = tid & 7, w = wave_id();
    const RlLds c = rl_carve(sm_raw, M);
    float* prow = c.rest;                                              // (16-byte aligned: rl_carve)
    float* inv_s = prow + D;
    unsigned long long* wb_k = reinterpret_cast<unsigned long long*>(inv_s + FR_THREADS);
    float* wb_v = reinterpret_cast<float*>(wb_k + 2 * NW);
    long long* p_id = reinterpret_cast<long long*>(wb_v + 2 * NW);
    float* p_inv = reinterpret_cast<float*>(p_id + 1);
    const float lam = a.lambda, oml = 1.0f - lam;

    for (int b = blockIdx.x; b < a.B; b += gridDim.x) {
        long long lo, len;
        rl_clamp_list(a.cand_off, a.n_cand, b, lo, len, tid == 0 ? a.flags : nullptr);
        const int u0 = a.unit_pre[b], nu = a.unit_pre[b + 1] - u0;     // (0: an empty list, or a row behind the cut of the prefix)
        __syncthreads();                                               // (the previous row's LDS is read)
        if (nu == 1) {
            for (int k = tid; k < M; k += FR_THREADS) { c.L.s[k] = a.part_s[(long long)u0 * M + k]; c.L.key[k] = a.part_k[(long long)u0 * M + k]; }
            __syncthreads();
        } else if (nu > 1) {
            rl_merge_units(c, M, a.part_s + (long long)u0 * M, a.part_k + (long long)u0 * M, nu);
        }
        // thread t: entry t of the shortlist
        const bool have = nu > 0 && tid < M;
        const unsigned long long key = have ? c.L.key[tid] : RL_KEY_NONE;
        const float r = have ? c.L.s[tid] : 0.f;
        bool alive = key != RL_KEY_NONE;
        const int n = __syncthreads_count(alive);                      // (the list is sorted: its entries are slots 0 .. n - 1)
        const long long id = (long long)(key >> 32), pos = (long long)(key & 0xffffffffull);
        float4 x[4][D / 16];
        {
            const float* row = a.table + (alive ? id : 0) * D;
#pragma unroll
            for (int g = 0; g < 4; ++g)
#pragma unroll
                for (int i = 0; i < D / 16; ++i) x[g][i] = alive ? ld4(row + g * DQ + 4 * i) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
        float my_inv = 1.0f;
        if (a.metric) {                                                // (uniform) eight lanes a row, as nb_norm_kernel
            for (int e0 = 0; e0 < n; e0 += FR_THREADS >> 3) {          // (uniform trip count: the exchanges need every lane)
                const int e = e0 + (tid >> 3);
                const float* row = e < n ? a.table + (long long)(c.L.key[e] >> 32) * D : nullptr;
                const float inv = sim_inv_norm<D>(row, part);
                if (part == 0 && e < n) inv_s[e] = inv;
            }
            __syncthreads();
            if (alive) my_inv = inv_s[tid];
        }
        const float lr = lam * r;
        float m = -INFINITY, v = lr;
        int j = 0;
        for (; j < K && j < n; ++j) {
            bool win = tid == 0;                                       // pick 1: the head of the shortlist
            if (j > 0) {
                float bv = -INFINITY;
                unsigned long long bk = RL_KEY_NONE;
                if (alive) {
                    v = lr - (oml * m);
                    if (v == v) { bv = v; bk = key; }
                }
                mm_wave_best(bv, bk);
                float* sv = wb_v + (j & 1) * NW;
                unsigned long long* sk = wb_k + (j & 1) * NW;
                if (lane_id() == 0) { sv[w] = bv; sk[w] = bk; }
                __syncthreads();
                bv = sv[0]; bk = sk[0];
#pragma unroll
                for (int i = 1; i < NW; ++i)
                    if (rl_before(sv[i], sk[i], bv, bk)) { bv = sv[i]; bk = sk[i]; }
                if (bk == RL_KEY_NONE) break;                          // (uniform) nothing remains
                win = alive && key == bk;
            }
            if (win) {
                const long long o = (long long)b * K + j;
                a.out_ids[o] = id;
                if (a.out_rel) a.out_rel[o] = r;
                if (a.out_value) a.out_value[o] = v;
                if (a.out_max_sim) a.out_max_sim[o] = j > 0 ? m : 0.f;
                if (a.out_pos) a.out_pos[o] = pos;
#pragma unroll
                for (int g = 0; g < 4; ++g)
#pragma unroll
                    for (int i = 0; i < D / 16; ++i) st4(prow + g * DQ + 4 * i, x[g][i]);
                *p_id = id; *p_inv = my_inv;
                alive = false;
            }
            __syncthreads();
            if (alive && id == *p_id) alive = false;                   // a duplicate of the pick
            if (alive) {
                float s = sim_dot_chain<D>(x, prow);
                if (a.metric) s = sim_cosine(s, my_inv, *p_inv);
                m = fmaxf(m, s);
            }
        }
        for (int k = j + tid; k < K; k += FR_THREADS) {
            const long long o = (long long)b * K + k;
            a.out_ids[o] = -1;
            if (a.out_rel) a.out_rel[o] = -INFINITY;
            if (a.out_value) a.out_value[o] = -INFINITY;
            if (a.out_max_sim) a.out_max_sim[o] = -INFINITY;
            if (a.out_pos) a.out_pos[o] = -1;
        }
    }
}

#pragma clang fp contract(fast)

// ---- host side ------------------------------------------------------------------------------------------------------------------------------
static inline bool mm_sizes_ok(int B, long long n_cand, int K, int M) {
    return B >= 1 && n_cand >= 0 && n_cand < 0x7fffffffLL && K >= 1 && K <= 256 && M >= 1 && M <= 256;
}

// workspace carve: unit_pre [B + 1] | part_s [unit bound][M] | part_k [unit bound][M] (8-byte keys)
static long long mm_workspace(int B, long long n_cand, int M, size_t* off_ps, size_t* off_pk) {
    size_t o = rl_align(((size_t)B + 1) * 4);
    const size_t rows = (size_t)rl_unit_bound(B, n_cand) * M;
    if (off_ps) *off_ps = o;
    o += rl_align(rows * 4);
    if (off_pk) *off_pk = o;
    o += rl_align(rows * 8);
    return (long long)o;
}

template <int D>
static int mm_launch(const MmArgs& a, hipStream_t st) {
    mm_prefix_kernel<<<1, FR_THREADS, 0, st>>>(a);
    AMID_LAUNCH_CHECK();
    if (a.n_cand > 0) {
        const int grid = (int)std::min(rl_unit_bound(a.B, a.n_cand), (long long)RL_GRID);
        mm_short_kernel<<<grid, FR_THREADS, rl_list_lds_bytes(a.M), st>>>(a);
        AMID_LAUNCH_CHECK();
    }
    mm_pick_kernel<D><<<std::min(a.B, RL_GRID), FR_THREADS, mm_pick_lds_bytes(D, a.M), st>>>(a);
    AMID_LAUNCH_CHECK();
    return AMID_OK;
}

}  // namespace amid

using namespace amid;

// (the carve has room for max(K, shortlist) slots a list, so the size falls with neither)
extern "C" long long amid_mmr_workspace_bytes(int B, long long n_cand, int D, int K, int shortlist) {
    if (!mm_sizes_ok(B, n_cand, K, shortlist) || (D != 64 && D != 128)) return -1;
    return mm_workspace(B, n_cand, std::max(K, shortlist), nullptr, nullptr);
}

extern "C" int amid_mmr_lists_f32(const long long* cand, const long long* cand_off, const float* rel, long long n_cand, int B,
                                  const float* table, long long n_rows, int D, int metric, float lambda, int K, int shortlist, void* ws,
                                  int* flags, long long* out_ids, float* out_rel, float* out_value, float* out_max_sim,
                                  long long* out_positions, void* stream) {
    AMID_CHECK_ARG(cand_off && table && ws && flags && out_ids);
    AMID_CHECK_ARG(mm_sizes_ok(B, n_cand, K, shortlist) && K <= shortlist && ((cand != nullptr && rel != nullptr) || n_cand == 0));
    AMID_CHECK_ARG(n_rows >= 1 && n_rows <= 0x7fffffffLL);
    AMID_CHECK_ARG(metric == 0 || metric == 1);
    AMID_CHECK_ARG(lambda >= 0.f && lambda <= 1.f);                    // (false for a NaN)
    if (D != 64 && D != 128) return AMID_ERR_UNSUPPORTED;
    MmArgs a{};
    a.cand = cand; a.cand_off = cand_off; a.rel = rel; a.n_cand = n_cand; a.table = table; a.n_rows = n_rows;
    a.B = B; a.D = D; a.metric = metric; a.K = K; a.M = shortlist; a.lambda = lambda;
    a.per = rl_per_for(B, n_cand, RL_UNITS);
    a.unit_bound = (int)std::min(rl_unit_bound(B, n_cand), 0x7fffffffLL);
    a.flags = flags;
    size_t o_ps = 0, o_pk = 0;
    mm_workspace(B, n_cand, shortlist, &o_ps, &o_pk);
    char* w = (char*)ws;
    a.unit_pre = (int*)w; a.part_s = (float*)(w + o_ps); a.part_k = (unsigned long long*)(w + o_pk);
    a.out_ids = out_ids; a.out_rel = out_rel; a.out_value = out_value; a.out_max_sim = out_max_sim; a.out_pos = out_positions;
    const hipStream_t st = (hipStream_t)stream;
    return D == 64 ? mm_launch<64>(a, st) : mm_launch<128>(a, st);
}
