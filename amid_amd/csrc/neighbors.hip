// Exact k-nearest neighbours of fp32 vectors: Q queries against the candidate rows of base [n_rows, D] by dot product or cosine, the k best
// of each query best first (ties to the lower id) -- "items similar to this item" over the item table, "users like this user" over stored
// user vectors.  Nothing of the Q x N score matrix reaches memory.
//
// Launches (all on the caller's stream, no host synchronisation):
//   nb_norm_kernel   (cosine) the inverse norm 1 / max(|row|, 1e-8) of every candidate and every query, once per call: eight lanes a row,
//                    each an fmaf chain over its D / 8 elements, joined by group_sum<8> -- a function of the row alone
//   nb_scan_kernel   a workgroup per (group of 16 qg queries, range of candidate tiles).  The queries are the B operand of
//                    v_mfma_f32_16x16x4_f32 and stay in registers for the whole walk: wave w holds queries 16 (w % qg) .. + 15, lane
//                    (j = lane & 15, gq = lane >> 4) elements [gq D/4, (gq + 1) D/4) of query j.  A tile of NB_TILE candidate rows goes
//                    through LDS once per workgroup (global -> registers one tile ahead -> LDS); its 16-row blocks are the A operand (float4 reads, k-slot gq walks the same contiguous
//                    range), two blocks = two independent accumulators at a time.  The 16 x 16 scores land in an LDS score tile; a query
//                    whose K-th entry some score reaches is flagged, and only flagged queries offer the tile to their running best-K list
//                    (topk_list.h's list and order; the merge of list + newcomers is its bitonic sort run by ONE wave, so the four waves
//                    serve four flagged queries at a time).
//   nb_merge_kernel  a workgroup per query: the ranges' lists through the same merge -> ids [Q, K], scores [Q, K]
//
// A score is a function of its two rows only.  The accumulator starts at 0 and takes D / 4 MFMAs in a fixed order; an MFMA is bitwise the
// fmaf chain over its k-slots 0 .. 3, so dot(a, b) = the chain over elements s, D/4 + s, 2 D/4 + s, 3 D/4 + s for s = 0 .. D/4 - 1, whatever the
// tile, the block, the wave or the pool.  Cosine multiplies by the two inverse norms in a fixed order.  Bit-identical rows therefore tie
// exactly, and the tie rule (lower id first) decides between them.
//
// Ids outside [0, n_rows) raise AMID_FLAG_INDEX_RANGE and are never dereferenced: such a candidate is absent (its LDS rows are zeros and it
// is never offered), such a query has no candidates (its list stays empty: padding).
#include <algorithm>
#include "topk_list.h"
#include "sim_parts.h"
#include "amid_hip.h"

namespace amid {

#pragma clang fp contract(off)

constexpr int NB_TILE = 128;            // candidate rows per tile
constexpr int NB_BLOCKS = NB_TILE / 16; // MFMA row blocks per tile
constexpr int NB_QMAX = 64;             // queries per workgroup at most (qg = 4 groups of 16)
constexpr int NB_WGS = 256;             // target workgroups of the scan: one per CU
constexpr int NB_LDSC = NB_TILE + 4;    // row stride of the score tile (floats)

struct NbArgs {
    const float* queries; const long long* query_ids; int Q;
    const float* base; long long n_rows;
    const long long* pool; long long n_cand;
    int metric, K, exclude_self;
    int qg;                                     // groups of 16 queries per workgroup: 4 (a group per wave) or 1 (the waves share the tile's blocks)
    int n_tiles, n_ranges, per;                 // tiles per range
    float* inv_c; float* inv_q;                 // workspace [n_cand], [Q] (cosine)
    float* part_s; int* part_i;                 // workspace [n_ranges][Q][K]
    int* flags; long long* out_ids; float* out_s;
};

__device__ __forceinline__ f32x4 nb_mfma(float a, float b, f32x4 c) { return sim_mfma(a, b, c); }       // (sim_parts.h: the arithmetic diversify.hip shares)
__device__ __forceinline__ bool nb_id_ok(const NbArgs& a, long long id) { return id >= 0 && id < a.n_rows; }

// ---- a wave's offer to a list ------------------------------------------------------------------------------------------------------------------
// The scan's offers run a wave a query (topk_list.h's fr_offer is a whole workgroup on one list, two barriers even when nothing beats it):
// the same rule and the same bitonic merge with the wave's own merge buffer, ordered by wave-level LDS fences only, so the four waves
// of the workgroup serve four queries at once.
__device__ __forceinline__ void nb_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Every lane of ONE wave calls this with two candidates (c0 / c1: it takes part).  Ss / Si: the wave's merge buffer [512] / [512].
__device__ __forceinline__ void nb_wave_offer(const FrList& L, float* Ss, int* Si, int K, bool c0, float s0, int id0, bool c1, float s1,
                                              int id1) {
    const int lane = lane_id();
    const int n = __builtin_amdgcn_readfirstlane(*L.n);
    bool b0 = c0, b1 = c1;
    if (n == K) {
        const float ks = L.s[K - 1];
        const int ki = L.id[K - 1];
        b0 = c0 && fr_before(s0, id0, ks, ki);
        b1 = c1 && fr_before(s1, id1, ks, ki);
    }
    const unsigned long long m0 = __ballot(b0), m1 = __ballot(b1);
    const int t0 = __popcll(m0), tot = t0 + __popcll(m1);
    if (tot == 0) return;                                      // (uniform in the wave)
    const int total = n + tot;                                 // (<= 256 + NB_TILE)
    int size = 2;
    while (size < total) size <<= 1;
    const unsigned long long lt = (1ull << lane) - 1ull;
    if (b0) { const int slot = n + __popcll(m0 & lt); Ss[slot] = s0; Si[slot] = id0; }
    if (b1) { const int slot = n + t0 + __popcll(m1 & lt); Ss[slot] = s1; Si[slot] = id1; }
    for (int i = lane; i < size; i += kWave) {
        if (i < n) { Ss[i] = L.s[i]; Si[i] = L.id[i]; }
        else if (i >= total) { Ss[i] = -INFINITY; Si[i] = FR_ID_NONE; }
    }
    nb_wave_sync();
    for (int k = 2, lk = 1; k <= size; k <<= 1, ++lk) {
        for (int j = k >> 1, lj = lk - 1; j > 0; j >>= 1, --lj) {             // (j = 1 << lj: the pair index without a division)
            for (int t = lane; t < (size >> 1); t += kWave) {
                const int i = ((t >> lj) << (lj + 1)) + (t & (j - 1)), l = i + j;
                const float sa = Ss[i], sb = Ss[l];
                const int ia = Si[i], ib = Si[l];
                const bool first = (i & k) == 0;               // this run ends up best-first
                if (first ? fr_before(sb, ib, sa, ia) : fr_before(sa, ia, sb, ib)) {
                    Ss[i] = sb; Ss[l] = sa; Si[i] = ib; Si[l] = ia;
                }
            }
            nb_wave_sync();
        }
    }
    const int keep = min(K, total);
    for (int i = lane; i < keep; i += kWave) { L.s[i] = Ss[i]; L.id[i] = Si[i]; }
    if (lane == 0) *L.n = keep;
    nb_wave_sync();
}

// ---- inverse norms --------------------------------------------------------------------------------------------------------------------------
template <int D>
__global__ __launch_bounds__(FR_THREADS) void nb_norm_kernel(const NbArgs a) {
    const int part = threadIdx.x & 7;
    const long long total = a.n_cand + a.Q;
    const long long stride = (long long)gridDim.x * (FR_THREADS >> 3);
    for (long long e0 = (long long)blockIdx.x * (FR_THREADS >> 3); e0 < total; e0 += stride) {      // (uniform trip count)
        const long long e = e0 + (threadIdx.x >> 3);
        const float* row = nullptr;
        if (e < a.n_cand) {
            const long long id = a.pool ? a.pool[e] : e;
            if (nb_id_ok(a, id)) row = a.base + id * D;
        } else if (e < total) {
            const long long q = e - a.n_cand;
            if (a.query_ids) {
                const long long id = a.query_ids[q];
                if (nb_id_ok(a, id)) row = a.base + id * D;
            } else {
                row = a.queries + q * D;
            }
        }
        const float inv = sim_inv_norm<D>(row, part);
        if (part == 0 && e < total) {
            if (e < a.n_cand) a.inv_c[e] = inv; else a.inv_q[e - a.n_cand] = inv;
        }
    }
}

// ---- scan -----------------------------------------------------------------------------------------------------------------------------------
// LDS (4-byte words): tile [NB_TILE][D + 4] | scores [16 qg][NB_LDSC] | lists [16 qg][K] scores | [16 qg][K] ids | n [16 qg] | thr [16 qg] |
// hit [16 qg] | qid [16 qg] | cid [NB_TILE] | cinv [NB_TILE] | a merge buffer per wave: [4][512 scores | 512 ids]
__host__ __device__ inline size_t nb_scan_lds_bytes(int D, int qg, int K) {
    const int nq = 16 * qg;
    return (size_t)4 * ((size_t)NB_TILE * (D + 4) + (size_t)nq * NB_LDSC + 2 * (size_t)nq * K + 4 * nq + 2 * NB_TILE + (FR_THREADS / kWave) * 2 * 512);
}

template <int D>
__global__ __launch_bounds__(FR_THREADS) void nb_scan_kernel(const NbArgs a) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    constexpr int LDA = D + 4, DQ = D / 4;
    const int K = a.K, tid = threadIdx.x, qg = a.qg, nq = 16 * qg;
    float* At = sm;
    float* sc = At + NB_TILE * LDA;
    float* ls = sc + nq * NB_LDSC;
    int* li = reinterpret_cast<int*>(ls + nq * K);
    int* ln = li + nq * K;
    float* thr = reinterpret_cast<float*>(ln + nq);
    int* hit = reinterpret_cast<int*>(thr + nq);
    int* qid = hit + nq;                                           // the query's own row (exclude_self), -1: none, -2: no such query
    int* cid = qid + nq;
    float* cinv = reinterpret_cast<float*>(cid + NB_TILE);

    const int lane = lane_id(), w = wave_id(), j = lane & 15, gq = lane >> 4;
    float* Ss = cinv + NB_TILE + w * 1024;                         // the wave's merge buffer
    int* Si = reinterpret_cast<int*>(Ss + 512);
    const int qgrp = w % qg, cpart = w / qg, cstep = 4 / qg;
    const long long q0 = (long long)blockIdx.x * nq;

    // the wave's queries: the B fragments of every MFMA of the walk
    const int qrow = qgrp * 16 + j;                                // row of the score tile and of the lists
    const long long q = q0 + qrow;
    const float* qp = nullptr;
    long long own = -2;
    if (q < a.Q) {
        if (a.query_ids) {
            const long long id = a.query_ids[q];
            if (nb_id_ok(a, id)) { qp = a.base + id * D; own = id; }
            else if (gq == 0 && cpart == 0 && blockIdx.y == 0) atomicOr(a.flags, AMID_FLAG_INDEX_RANGE);
        } else {
            qp = a.queries + q * D; own = -1;
        }
    }
    float qf[DQ];
#pragma unroll
    for (int s4 = 0; s4 < DQ / 4; ++s4) {
        const float4 v = qp ? ld4(qp + gq * DQ + 4 * s4) : make_float4(0.f, 0.f, 0.f, 0.f);
        qf[4 * s4] = v.x; qf[4 * s4 + 1] = v.y; qf[4 * s4 + 2] = v.z; qf[4 * s4 + 3] = v.w;
    }
    const float qinv = (a.metric && qp) ? a.inv_q[q] : 1.0f;
    if (gq == 0 && cpart == 0) { qid[qrow] = (int)own; ln[qrow] = 0; }

    // A tile's rows travel global -> registers -> LDS: thread tid carries float4 (tid % DQ) of rows i RPI + tid / DQ.  The next tile's loads
    // are issued before this tile's products and land in LDS after its offers, so they are in flight behind the MFMAs and the merges.
    constexpr int NPRE = NB_TILE * DQ / FR_THREADS, RPI = FR_THREADS / DQ;
    float4 pre[NPRE];
    unsigned pre_ok = 0;                                           // bit i: pre[i] is a candidate's row (else: zeros go to LDS)
    const int pr = tid / DQ, pc4 = tid - pr * DQ;
    // (every load is unconditional, so that they all go out back to back: an absent candidate reads pool slot n_cand - 1 / row 0 instead --
    // never the address its bad id would give -- and its bit in pre_ok stays clear)
    auto issue = [&](int t) {
        const long long n0 = (long long)t * NB_TILE;
        long long ids[NPRE];
#pragma unroll
        for (int i = 0; i < NPRE; ++i) {
            const long long n = min(n0 + i * RPI + pr, a.n_cand - 1);
            ids[i] = a.pool ? a.pool[n] : n;
        }
        pre_ok = 0;
#pragma unroll
        for (int i = 0; i < NPRE; ++i) {
            const bool ok = n0 + i * RPI + pr < a.n_cand && nb_id_ok(a, ids[i]);
            pre_ok |= ok ? 1u << i : 0u;
            pre[i] = ld4(a.base + (ok ? ids[i] : 0) * D + 4 * pc4);
        }
    };
    const int t0 = blockIdx.y * a.per, t1 = min(a.n_tiles, t0 + a.per);
    if (t0 < t1) issue(t0);
    for (int t = t0; t < t1; ++t) {
        const long long n0 = (long long)t * NB_TILE;
        const int nn = (int)min((long long)NB_TILE, a.n_cand - n0);
        __syncthreads();                                               // (every wave's products and offers of the previous tile are done; first tile: qid, ln written)
        if (tid < NB_TILE) {
            long long id = -1;
            if (tid < nn) {
                id = a.pool ? a.pool[n0 + tid] : n0 + tid;
                if (!nb_id_ok(a, id)) { atomicOr(a.flags, AMID_FLAG_INDEX_RANGE); id = -1; }
            }
            cid[tid] = (int)id;
            cinv[tid] = (a.metric && id >= 0) ? a.inv_c[n0 + tid] : 1.0f;
        } else if (tid - NB_TILE < nq) {
            const int i = tid - NB_TILE;
            hit[i] = 0;
            thr[i] = ln[i] == K ? ls[i * K + K - 1] : -INFINITY;
        }
#pragma unroll
        for (int i = 0; i < NPRE; ++i)
            st4(At + (i * RPI + pr) * LDA + 4 * pc4, (pre_ok >> i) & 1u ? pre[i] : make_float4(0.f, 0.f, 0.f, 0.f));
        __syncthreads();
        if (t + 1 < t1) issue(t + 1);
        const float th = thr[qrow];
        for (int blk = cpart; blk < NB_BLOCKS; blk += 2 * cstep) {     // two blocks a pass: blk and blk + cstep
            if (blk * 16 >= nn) break;                                  // (uniform in the wave)
            const float* A0 = At + (blk * 16 + j) * LDA + gq * DQ;
            const float* A1 = A0 + cstep * 16 * LDA;
            f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int s4 = 0; s4 < DQ / 4; ++s4) {
                const float4 x = ld4(A0 + 4 * s4), y = ld4(A1 + 4 * s4);
                acc0 = nb_mfma(x.x, qf[4 * s4], acc0);     acc1 = nb_mfma(y.x, qf[4 * s4], acc1);
                acc0 = nb_mfma(x.y, qf[4 * s4 + 1], acc0); acc1 = nb_mfma(y.y, qf[4 * s4 + 1], acc1);
                acc0 = nb_mfma(x.z, qf[4 * s4 + 2], acc0); acc1 = nb_mfma(y.z, qf[4 * s4 + 2], acc1);
                acc0 = nb_mfma(x.w, qf[4 * s4 + 3], acc0); acc1 = nb_mfma(y.w, qf[4 * s4 + 3], acc1);
            }
            // lane: query j, candidates 4 gq + r of each block
            const int c0 = blk * 16 + 4 * gq, c1 = c0 + cstep * 16;
            float4 s0 = make_float4(acc0[0], acc0[1], acc0[2], acc0[3]), s1 = make_float4(acc1[0], acc1[1], acc1[2], acc1[3]);
            if (a.metric) {
                const float4 i0 = ld4(cinv + c0), i1 = ld4(cinv + c1);
                s0 = make_float4(sim_cosine(s0.x, qinv, i0.x), sim_cosine(s0.y, qinv, i0.y), sim_cosine(s0.z, qinv, i0.z), sim_cosine(s0.w, qinv, i0.w));
                s1 = make_float4(sim_cosine(s1.x, qinv, i1.x), sim_cosine(s1.y, qinv, i1.y), sim_cosine(s1.z, qinv, i1.z), sim_cosine(s1.w, qinv, i1.w));
            }
            st4(sc + qrow * NB_LDSC + c0, s0);
            st4(sc + qrow * NB_LDSC + c1, s1);
            const bool below = s0.x < th && s0.y < th && s0.z < th && s0.w < th && s1.x < th && s1.y < th && s1.z < th && s1.w < th;
            if (!below && qp != nullptr) hit[qrow] = 1;                  // (every writer stores the same value; an absent query offers nothing)
        }
        __syncthreads();
        // the flagged queries, dealt to the waves: lane l offers candidates l and l + 64 of the tile
        const bool on0 = lane < nn, on1 = lane + kWave < nn;
        const int id0 = on0 ? cid[lane] : -1, id1 = on1 ? cid[lane + kWave] : -1;
        for (int i = w; i < nq; i += FR_THREADS / kWave) {
            if (__builtin_amdgcn_readfirstlane(hit[i]) == 0) continue;
            const int own_i = __builtin_amdgcn_readfirstlane(qid[i]);
            const bool live = own_i != -2;
            const bool c0 = live && id0 >= 0 && !(a.exclude_self && id0 == own_i);
            const bool c1 = live && id1 >= 0 && !(a.exclude_self && id1 == own_i);
            const float s0 = sc[i * NB_LDSC + lane], s1 = sc[i * NB_LDSC + lane + kWave];
            const FrList L{ls + i * K, li + i * K, ln + i};
            nb_wave_offer(L, Ss, Si, K, c0, s0, id0, c1, s1, id1);
        }
    }
    __syncthreads();
    for (int i = 0; i < nq; ++i) {
        if (q0 + i >= a.Q) break;
        const int n = ln[i];
        const long long o = ((long long)blockIdx.y * a.Q + q0 + i) * K;
        for (int k = tid; k < K; k += FR_THREADS) {
            a.part_s[o + k] = k < n ? ls[i * K + k] : -INFINITY;
            a.part_i[o + k] = k < n ? li[i * K + k] : FR_ID_NONE;
        }
    }
}

__global__ __launch_bounds__(FR_THREADS) void nb_merge_kernel(const NbArgs a) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    fr_merge_ranges(sm, a.K, a.n_ranges, a.Q, blockIdx.x, a.part_s, a.part_i, a.out_ids, a.out_s);
}

#pragma clang fp contract(fast)

// ---- host side ------------------------------------------------------------------------------------------------------------------------------
static inline size_t nb_align(size_t x) { return (x + 255) & ~(size_t)255; }
static inline long long nb_tiles(long long n_cand) { return (n_cand + NB_TILE - 1) / NB_TILE; }
static inline int nb_qg(int Q, int k) { return (k > 64 || Q <= 16) ? 1 : NB_QMAX / 16; }

// rows [K] of the per-range lists: an upper bound of n_ranges * Q that does not fall when Q, n_cand or k grows (n_ranges * Q itself does,
// where one more query starts another workgroup and halves the ranges)
static inline size_t nb_part_rows(int Q, long long n_cand) {
    const size_t g16 = ((size_t)Q + 15) / 16;
    return std::min(((size_t)NB_WGS + g16) * NB_QMAX, (size_t)nb_tiles(n_cand) * g16 * NB_QMAX);
}

// workspace carve: inv_c [n_cand] | inv_q [Q] | part_s [rows][k] | part_i [rows][k]
static long long nb_workspace(int Q, long long n_cand, int k, size_t* off_q, size_t* off_ps, size_t* off_pi) {
    size_t o = nb_align((size_t)n_cand * 4);
    if (off_q) *off_q = o;
    o += nb_align((size_t)Q * 4);
    const size_t part = nb_part_rows(Q, n_cand) * k * 4;
    if (off_ps) *off_ps = o;
    o += nb_align(part);
    if (off_pi) *off_pi = o;
    o += nb_align(part);
    return (long long)o;
}

// the scan's target workgroup count: NB_WGS, or what amid_neighbors_target_workgroups set (tests: fewer workgroups = longer ranges)
static int nb_target_wgs = NB_WGS;

static inline bool nb_sizes_ok(int Q, long long n_cand, int k) { return Q >= 1 && n_cand >= 1 && n_cand < 0x7fffffffLL && k >= 1 && k <= 256; }

template <int D>
static int nb_launch(const NbArgs& a, hipStream_t st) {
    static unsigned long long done_scan = 0, done_merge = 0;
    if (a.metric) {
        const long long groups = (a.n_cand + a.Q + (FR_THREADS >> 3) - 1) / (FR_THREADS >> 3);
        nb_norm_kernel<D><<<(int)std::min(groups, (long long)4096), FR_THREADS, 0, st>>>(a);
        AMID_LAUNCH_CHECK();
    }
    if (int rc = lds_attr_once((const void*)nb_scan_kernel<D>, 160 * 1024, done_scan)) return rc;
    const int n_qwg = (a.Q + 16 * a.qg - 1) / (16 * a.qg);
    nb_scan_kernel<D><<<dim3(n_qwg, a.n_ranges), FR_THREADS, nb_scan_lds_bytes(D, a.qg, a.K), st>>>(a);
    AMID_LAUNCH_CHECK();
    if (int rc = lds_attr_once((const void*)nb_merge_kernel, 160 * 1024, done_merge)) return rc;
    nb_merge_kernel<<<a.Q, FR_THREADS, fr_merge_lds_bytes(a.K), st>>>(a);
    AMID_LAUNCH_CHECK();
    return AMID_OK;
}

}  // namespace amid

using namespace amid;

extern "C" long long amid_neighbors_workspace_bytes(int Q, long long n_cand, int D, int k) {
    if (!nb_sizes_ok(Q, n_cand, k) || (D != 64 && D != 128)) return -1;
    return nb_workspace(Q, n_cand, k, nullptr, nullptr, nullptr);
}

extern "C" int amid_neighbors_target_workgroups(int wgs) {
    const int before = nb_target_wgs;
    nb_target_wgs = wgs >= 1 ? std::min(wgs, NB_WGS) : NB_WGS;
    return before;
}

extern "C" int amid_neighbors_f32(const float* queries, const long long* query_ids, int Q, const float* base, long long n_rows, int D,
                                  const long long* pool, long long n_pool, int metric, int k, int exclude_self, void* workspace, int* flags,
                                  long long* ids, float* scores, void* stream) {
    AMID_CHECK_ARG(base && workspace && flags && ids && scores);
    AMID_CHECK_ARG((queries != nullptr) != (query_ids != nullptr));
    AMID_CHECK_ARG(!exclude_self || query_ids != nullptr);
    AMID_CHECK_ARG(metric == 0 || metric == 1);
    AMID_CHECK_ARG(n_rows >= 1 && n_rows < 0x7fffffffLL && (pool == nullptr || n_pool >= 1));
    const long long n_cand = pool ? n_pool : n_rows;
    AMID_CHECK_ARG(nb_sizes_ok(Q, n_cand, k));
    if (D != 64 && D != 128) return AMID_ERR_UNSUPPORTED;
    NbArgs a{};
    a.queries = queries; a.query_ids = query_ids; a.Q = Q; a.base = base; a.n_rows = n_rows; a.pool = pool; a.n_cand = n_cand;
    a.metric = metric; a.K = k; a.exclude_self = exclude_self ? 1 : 0; a.flags = flags; a.out_ids = ids; a.out_s = scores;
    a.qg = nb_qg(Q, k);
    const int n_qwg = (Q + 16 * a.qg - 1) / (16 * a.qg);
    a.n_tiles = (int)nb_tiles(n_cand);
    const int want = std::max(1, std::min(a.n_tiles, (nb_target_wgs + n_qwg - 1) / n_qwg));
    a.per = (a.n_tiles + want - 1) / want;
    a.n_ranges = (a.n_tiles + a.per - 1) / a.per;                      // (no empty range)
    size_t o_q = 0, o_ps = 0, o_pi = 0;
    nb_workspace(Q, n_cand, k, &o_q, &o_ps, &o_pi);
    char* ws = (char*)workspace;
    a.inv_c = (float*)ws; a.inv_q = (float*)(ws + o_q); a.part_s = (float*)(ws + o_ps); a.part_i = (int*)(ws + o_pi);
    const hipStream_t st = (hipStream_t)stream;
    return D == 64 ? nb_launch<64>(a, st) : nb_launch<128>(a, st);
}
