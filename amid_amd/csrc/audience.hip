// Audience top-K: for each of Q query items, the K stored user vectors that predictModule scores highest for it -- full_rank.hip's question
// the other way round ("which users for this item").  p(u, c) = sigmoid(w2 . relu((W1[:, :D] u + b1) + W1[:, D:] E[c]) + b2).
//
// The candidates are rows of a vector matrix V [N, D] (encode_users' output, say), each of domain 0 or 1; the host hands over the ascending
// row lists of the two domains (slots_d1, slots_d2: the counterpart of full_rank.hip's two item pools).  The user half W1[:, :D] V[r] + b1
// does not depend on the item: it is formed ONCE per listed row, and per (row, item) pair only hid (add, max, fma) and the logit's tree
// remain.  Every piece is head_parts.h's (the user half: user_half_chain's fmas joined by group_sum<8>, then + b1[j], as fr_user_kernel
// forms it; the item half: item_half_chain joined by group_sum<8>, as fr_items_kernel forms it; head_logit_p adds the two with one commutative
// fp32 addition): a score is bit-identical to what amid_topk_f32 gives for the same vector and the same table row.
//
// Launches (all on the caller's stream, no host synchronisation):
//   au_halves_kernel  (amid_audience_halves_f32) persistent workgroups over tiles of 256 listed rows: W1[:, :D]^T staged in LDS once per
//                     workgroup; 64 rows at a time travel global -> LDS by coalesced 16-byte loads; eight lanes a row, lane `part` keeps
//                     elements part, part + 8, .. of two rows in registers and walks the hid outputs four at a time -- one 16-byte LDS read of W1^T
//                     per eight fmas
//   au_query_kernel   (amid_audience_topk_f32) the item halves of the Q query rows of the table, eight lanes an output
//   au_topk_kernel    a workgroup per (group of AU_QB queries, range of tiles): a thread per candidate row of the tile with its hid values in
//                     registers; the group's queries of the tile's domain stream past; a running best-K list per query in LDS
//                     (topk_list.h's list, order and merge; the merges deferred: au_offer)
//   au_merge_kernel   a workgroup per query: the ranges' lists through the same merge -> rows [Q, K], scores [Q, K]
// The exclusion list of a query (holders: ascending row indices, a CSR over the queries) is applied where its rows fall: a tile finds the
// list's first entry inside its row range by binary search and marks the entries up to its last row.  No (query, candidate) pair is
// tested against a list.
#include <algorithm>
#include "head_parts.h"
#include "topk_list.h"
#include "amid_hip.h"

namespace amid {

#pragma clang fp contract(off)

constexpr int AU_TILE = 256;            // candidate rows per tile: one per thread of the top-K launch
constexpr int AU_SUB = 64;              // rows the halves launch stages in LDS at a time: two per group of eight lanes
constexpr int AU_QB = 8;               // queries per top-K workgroup
constexpr int AU_PEND = 256;            // newcomers a query collects between two merges into its list (list + pending <= the 512 of the merge buffer)
constexpr int AU_GRID = 512;            // persistent workgroups of the halves launch
constexpr int AU_TOPK_WGS = 1024;       // target workgroups of the top-K launch

struct AuArgs {
    const float* v; long long n_vectors;        // V [n_vectors][D]
    const int* slots[2]; int n[2]; int n_tiles[2];      // ascending rows of each domain
    const long long* items; const long long* item_dom; int Q;
    const float* table; long long n_rows;
    const float* w1; const float* b1; const float* w2; const float* b2;
    const int* hold; const long long* hold_off; // holders(q) = hold[hold_off[q] .. hold_off[q + 1]), ascending; or hold null
    int D, hid, K;
    int* flags;
    float* uh;                                  // workspace [n0 + n1][hid]
    float* qh;                                  // workspace [Q][hid]
    float* part_s; int* part_i; int n_ranges;   // workspace [n_ranges][Q][K]
    long long* out_rows; float* out_s;          // [Q][K]
};

__device__ __forceinline__ void au_tile_of(const AuArgs& a, int t, int& dom, int& n0, int& nn) {
    dom = t < a.n_tiles[0] ? 0 : 1;
    n0 = (dom ? t - a.n_tiles[0] : t) * AU_TILE;
    nn = min(AU_TILE, a.n[dom] - n0);
}

// ---- user halves of every listed row --------------------------------------------------------------------------------------------------------
// LDS (floats): w1t [D][HID + 4] | rows [AU_SUB][D + 8]  (row stride D + 8: the eight rows of a wave start eight banks apart; w1t's stride
// HID + 4 keeps its rows 16-byte aligned and the eight lanes' 16-byte reads of one output quad on disjoint banks for HID 16 / 32 / 64)
__host__ __device__ inline size_t au_halves_lds_bytes(int D, int hid) { return (size_t)4 * ((size_t)D * (hid + 4) + (size_t)AU_SUB * (D + 8)); }

// user_half_chain (head_parts.h) for four consecutive outputs j0 .. j0 + 3 and two rows at once, the lane's elements already in registers
// (u[i] = row[part + 8 i], D = 8 NE): w = w1t + j0, one 16-byte LDS read per element feeds the eight chains.  Each chain is its output's own,
// acc = fmaf(w[e ldw], u[e], acc) over e = part, part + 8, ..: user_half_chain's fmas in user_half_chain's order.
template <int NE>
__device__ __forceinline__ void au_user_half_chains4(const float* __restrict__ w, int ldw, const float (&u0)[NE], const float (&u1)[NE], int part,
                                                     float (&a0)[4], float (&a1)[4]) {
#pragma unroll
    for (int c = 0; c < 4; ++c) { a0[c] = 0.f; a1[c] = 0.f; }
#pragma unroll
    for (int i = 0; i < NE; ++i) {
        const float4 wv = ld4(w + (part + 8 * i) * ldw);
        a0[0] = fmaf(wv.x, u0[i], a0[0]); a0[1] = fmaf(wv.y, u0[i], a0[1]); a0[2] = fmaf(wv.z, u0[i], a0[2]); a0[3] = fmaf(wv.w, u0[i], a0[3]);
        a1[0] = fmaf(wv.x, u1[i], a1[0]); a1[1] = fmaf(wv.y, u1[i], a1[1]); a1[2] = fmaf(wv.z, u1[i], a1[2]); a1[3] = fmaf(wv.w, u1[i], a1[3]);
    }
}

template <int HID, int D>
__global__ __launch_bounds__(FR_THREADS) void au_halves_kernel(const AuArgs a) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    constexpr int LDW = HID + 4, LDU = D + 8, NE = D / 8, Q4 = D / 4;
    float* w1t = sm;                                                   // W1[:, :D]^T
    float* us = w1t + D * LDW;                                         // (16-byte aligned: D LDW is a multiple of 4)
    const int tid = threadIdx.x, part = tid & 7, g = tid >> 3;
    for (int x = tid; x < HID * D; x += FR_THREADS) {
        const int j = x / D, e = x - j * D;
        w1t[e * LDW + j] = a.w1[(long long)j * 2 * D + e];
    }
    const int n_t = a.n_tiles[0] + a.n_tiles[1];
    for (int t = blockIdx.x; t < n_t; t += gridDim.x) {
        int dom, n0, nn;
        au_tile_of(a, t, dom, n0, nn);
        const int* slots = a.slots[dom];
        const long long base = (long long)(dom ? a.n[0] : 0) + n0;
        for (int sub = 0; sub < nn; sub += AU_SUB) {
            const int ns = min(AU_SUB, nn - sub);
            __syncthreads();                                           // (w1t staged; the previous rows read)
#pragma unroll
            for (int x0 = 0; x0 < AU_SUB * Q4; x0 += FR_THREADS) {
                const int x = x0 + tid, n = x / Q4, c4 = x - n * Q4;
                float4 val = make_float4(0.f, 0.f, 0.f, 0.f);
                if (n < ns) {
                    long long r = slots[n0 + sub + n];
                    if (r < 0 || r >= a.n_vectors) {                   // (raises the index flag and reads row 0: the half is never used)
                        if (c4 == 0) atomicOr(a.flags, AMID_FLAG_INDEX_RANGE);
                        r = 0;
                    }
                    val = ld4(a.v + r * D + 4 * c4);
                }
                st4(us + n * LDU + 4 * c4, val);
            }
            __syncthreads();
            float u0[NE], u1[NE];                                      // rows g and g + 32 of the staged 64
#pragma unroll
            for (int i = 0; i < NE; ++i) { u0[i] = us[g * LDU + part + 8 * i]; u1[i] = us[(g + 32) * LDU + part + 8 * i]; }
            float* o0 = a.uh + (base + sub + g) * HID;
            float* o1 = o0 + 32 * HID;
            for (int j0 = 0; j0 < HID; j0 += 4) {
                float a0[4], a1[4];
                au_user_half_chains4<NE>(w1t + j0, LDW, u0, u1, part, a0, a1);
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const int j = j0 + c;
                    const float s0 = group_sum<8>(a0[c]), s1 = group_sum<8>(a1[c]);
                    if (part == (j & 7)) {                             // (every lane of the eight holds the sum: they share the stores)
                        const float bj = a.b1[j];
                        if (g < ns) o0[j] = s0 + bj;
                        if (g + 32 < ns) o1[j] = s1 + bj;
                    }
                }
            }
        }
    }
}

// ---- item halves of the queries -----------------------------------------------------------------------------------------------------------------
// An id outside the table raises the index flag and reads row 0 (the query's row of the result is never used).
template <int HID>
__global__ __launch_bounds__(FR_THREADS) void au_query_kernel(const AuArgs a) {
    const int D = a.D, tid = threadIdx.x, part = tid & 7;
    const int nj = blockIdx.x * (FR_THREADS >> 3) + (tid >> 3);
    const int q = nj / HID, j = nj - q * HID;
    const bool on = q < a.Q;
    float acc = 0.f;
    if (on) {
        long long id = a.items[q];
        if (id < 0 || id >= a.n_rows) {
            if (part == 0 && j == 0) atomicOr(a.flags, AMID_FLAG_INDEX_RANGE);
            id = 0;
        }
        acc = item_half_chain(a.w1 + (long long)j * 2 * D + D, 1, a.table + id * D, D, part);
    }
    acc = group_sum<8>(acc);
    if (on && part == 0) a.qh[(long long)q * HID + j] = acc;
}

// ---- top-K ----------------------------------------------------------------------------------------------------------------------------------
// LDS (4-byte words): lists [AU_QB][K] scores | [AU_QB][K] rows | n [AU_QB] | merge [512] scores | [512] rows | wcnt [4] | ex [AU_TILE] |
// tile rows [AU_TILE] | pending [AU_QB][AU_PEND] scores | [AU_QB][AU_PEND] rows | pending n [AU_QB]
__host__ __device__ inline size_t au_topk_lds_bytes(int K) {
    return (size_t)4 * (2 * AU_QB * K + AU_QB + 2 * 512 + 4 + 2 * AU_TILE + 2 * AU_QB * AU_PEND + AU_QB);
}

// A query's running list with its pending newcomers.  fr_offer sorts list + newcomers for every tile that carries one, and in a long
// range nearly every tile does (about K / t of the t-th tile's candidates beat the K-th entry).  Here the newcomers that beat the list's
// K-th entry AS IT STANDS collect in a pending buffer and are merged (fr_sort_keep) only when the next tile's might not fit, and at the
// end of the range.  The K-th entry only rises at a merge, so between merges the test lets through a superset of what a fresh list would:
// the k best and their order are the same.  A list that is not full yet merges at once (it has no K-th entry to test against).
struct AuPending { float* s; int* id; int* n; };

// merge the pn pending newcomers into the list (every thread of the workgroup; pn uniform)
__device__ __forceinline__ void au_flush(const FrList& L, const FrScratch& S, const AuPending& P, int K, int pn) {
    __syncthreads();                                                   // (the pending entries are written)
    const int n = *L.n;
    for (int x = threadIdx.x; x < pn; x += FR_THREADS) { S.s[n + x] = P.s[x]; S.id[n + x] = P.id[x]; }
    if (threadIdx.x == 0) *P.n = 0;
    fr_sort_keep(L, S, K, n, n + pn);                                  // (n + pn <= K + AU_PEND <= 512)
}

// fr_offer's contract with the merge deferred: one candidate per thread (cand: it takes part); every thread of the workgroup calls this
__device__ __forceinline__ void au_offer(const FrList& L, const FrScratch& S, const AuPending& P, int K, bool cand, float s, int id) {
    const int tid = threadIdx.x, lane = lane_id(), w = tid >> 6;
    const int n = *L.n;
    int pn = *P.n;
    bool beat = cand;
    if (cand && n == K) beat = fr_before(s, id, L.s[K - 1], L.id[K - 1]);
    const unsigned long long m = __ballot(beat);
    if (lane == 0) S.wcnt[w] = __popcll(m);
    __syncthreads();
    int off = 0, tot = 0;
    for (int v = 0; v < FR_THREADS / 64; ++v) { off += v < w ? S.wcnt[v] : 0; tot += S.wcnt[v]; }
    __syncthreads();                                           // (every wave has read the counts, n and pn before anything below writes them)
    if (tot == 0) return;                                      // (uniform)
    if (pn + tot > AU_PEND) { au_flush(L, S, P, K, pn); pn = 0; }      // (uniform; the newcomers were tested against the older, lower K-th entry)
    if (beat) {
        const int slot = pn + off + __popcll(m & ((1ull << lane) - 1ull));
        P.s[slot] = s; P.id[slot] = id;
    }
    if (n < K) au_flush(L, S, P, K, pn + tot);                 // (pn is 0 here: a list that is not full never leaves anything pending)
    else if (tid == 0) *P.n = pn + tot;
}

template <int HID>
__global__ __launch_bounds__(FR_THREADS) void au_topk_kernel(const AuArgs a) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int K = a.K, tid = threadIdx.x;
    float* ls = sm;
    int* li = reinterpret_cast<int*>(ls + AU_QB * K);
    int* ln = li + AU_QB * K;
    FrScratch S;
    S.s = reinterpret_cast<float*>(ln + AU_QB);
    S.id = reinterpret_cast<int*>(S.s + 512);
    S.wcnt = S.id + 512;
    int* ex = S.wcnt + 4;
    int* ids_s = ex + AU_TILE;
    float* pend_s = reinterpret_cast<float*>(ids_s + AU_TILE);
    int* pend_i = reinterpret_cast<int*>(pend_s + AU_QB * AU_PEND);
    int* pend_n = pend_i + AU_QB * AU_PEND;
    const int q0 = blockIdx.x * AU_QB, nq = min(AU_QB, a.Q - q0);
    const int r = blockIdx.y;
    const int n_t = a.n_tiles[0] + a.n_tiles[1];
    const int per = (n_t + a.n_ranges - 1) / a.n_ranges;
    const int t0 = r * per, t1 = min(n_t, t0 + per);
    if (tid < AU_QB) { ln[tid] = 0; pend_n[tid] = 0; }
    for (int t = t0; t < t1; ++t) {
        int dom, n0, nn;
        au_tile_of(a, t, dom, n0, nn);
        const bool on = tid < nn;
        const int id = on ? a.slots[dom][n0 + tid] : FR_ID_NONE;
        __syncthreads();                                               // (the previous tile's searches of ids_s are done)
        ids_s[tid] = id;
        float c[HID];
        const float* cr = a.uh + ((long long)(dom ? a.n[0] : 0) + n0 + (on ? tid : 0)) * HID;
#pragma unroll
        for (int j = 0; j < HID; ++j) c[j] = cr[j];
        for (int i = 0; i < nq; ++i) {
            const int q = q0 + i;
            if ((a.item_dom[q] != 0 ? 1 : 0) != dom) continue;         // (uniform)
            ex[tid] = 0;
            __syncthreads();                                           // (ids_s and ex written; the previous query's offer has read ex)
            if (a.hold != nullptr) {
                const long long lo = a.hold_off[q], hi = a.hold_off[q + 1];
                const int first = ids_s[0], last = ids_s[nn - 1];
                long long l = lo, h = hi;                              // the list's first entry >= the tile's first row (uniform)
                while (l < h) { const long long mid = (l + h) >> 1; if (a.hold[mid] < first) l = mid + 1; else h = mid; }
                for (long long k = l + tid; k < hi; k += FR_THREADS) {
                    const int o = a.hold[k];
                    if (o > last) break;
                    int x = 0, y = nn;
                    while (x < y) { const int mid = (x + y) >> 1; if (ids_s[mid] < o) x = mid + 1; else y = mid; }
                    if (x < nn && ids_s[x] == o) ex[x] = 1;
                }
                __syncthreads();
            }
            const float* qhq = a.qh + (long long)q * HID;
            const float p = head_logit_p<HID>([&](int j) { return c[j]; }, [&](int j) { return qhq[j]; }, a.w2, a.b2[0]);
            const FrList L{ls + i * K, li + i * K, ln + i};
            const AuPending P{pend_s + i * AU_PEND, pend_i + i * AU_PEND, pend_n + i};
            au_offer(L, S, P, K, on && ex[tid] == 0, p, id);
        }
    }
    __syncthreads();
    for (int i = 0; i < nq; ++i) {                                     // what is still pending
        const int pn = pend_n[i];
        if (pn == 0) continue;                                         // (uniform)
        const FrList L{ls + i * K, li + i * K, ln + i};
        const AuPending P{pend_s + i * AU_PEND, pend_i + i * AU_PEND, pend_n + i};
        au_flush(L, S, P, K, pn);
    }
    for (int i = 0; i < nq; ++i) {
        const int n = ln[i];
        const long long o = ((long long)r * a.Q + q0 + i) * K;
        for (int k = tid; k < K; k += FR_THREADS) {
            a.part_s[o + k] = k < n ? ls[i * K + k] : -INFINITY;
            a.part_i[o + k] = k < n ? li[i * K + k] : FR_ID_NONE;
        }
    }
}

__global__ __launch_bounds__(FR_THREADS) void au_merge_kernel(const AuArgs a) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    fr_merge_ranges(sm, a.K, a.n_ranges, a.Q, blockIdx.x, a.part_s, a.part_i, a.out_rows, a.out_s);
}

#pragma clang fp contract(fast)

// ---- host side ------------------------------------------------------------------------------------------------------------------------------
static inline int au_tiles(int n) { return (n + AU_TILE - 1) / AU_TILE; }
static inline int au_qgroups(int Q) { return (Q + AU_QB - 1) / AU_QB; }
// the top-K launch's target workgroup count: AU_TOPK_WGS, or what amid_audience_target_workgroups set (tests: fewer workgroups = longer ranges)
static int au_target_wgs = AU_TOPK_WGS;
static inline int au_ranges(int Q, int n_tiles) { return std::max(1, std::min(n_tiles, (au_target_wgs + au_qgroups(Q) - 1) / au_qgroups(Q))); }
static inline size_t au_align(size_t x) { return (x + 255) & ~(size_t)255; }

// rows [K] of the per-range lists: an upper bound of n_ranges * Q that does not fall when Q or either n grows (n_ranges * Q itself does,
// where one more query starts another workgroup and the ranges get fewer): n_ranges <= AU_TOPK_WGS / groups + 1 (whatever the target
// amid_audience_target_workgroups set: it is at most AU_TOPK_WGS) and <= n_tiles
static inline size_t au_part_rows(int Q, int n_tiles) {
    const size_t g = (size_t)au_qgroups(Q);
    return std::min(((size_t)AU_TOPK_WGS + g) * AU_QB, (size_t)n_tiles * g * AU_QB);
}

static inline bool au_sizes_ok(int Q, int n1, int n2, int k) {
    return Q >= 1 && k >= 1 && k <= 256 && n1 >= 0 && n2 >= 0 && (long long)n1 + n2 >= 1 && (long long)n1 + n2 < 0x7fffffffLL;
}
static inline bool au_shape_ok(int D, int hid) { return (D == 64 || D == 128) && (hid == 16 || hid == 32 || hid == 64); }

// workspace carve: uh [n1 + n2][hid] | qh [Q][hid] | part_s [rows][k] | part_i [rows][k]  (uh first: where it lies depends on nothing else,
// so the halves launch serves every later Q and k)
static long long au_workspace(int Q, int n1, int n2, int hid, int k, size_t* off_qh, size_t* off_ps, size_t* off_pi) {
    size_t o = au_align(((size_t)n1 + n2) * hid * 4);
    if (off_qh) *off_qh = o;
    o += au_align((size_t)Q * hid * 4);
    const size_t part = au_part_rows(Q, au_tiles(n1) + au_tiles(n2)) * k * 4;
    if (off_ps) *off_ps = o;
    o += au_align(part);
    if (off_pi) *off_pi = o;
    o += au_align(part);
    return (long long)o;
}

template <int HID, int D>
static int au_halves_launch(const AuArgs& a, hipStream_t st) {
    static unsigned long long done = 0;
    const size_t lds = au_halves_lds_bytes(D, HID);
    if (int rc = lds_attr_once((const void*)au_halves_kernel<HID, D>, 160 * 1024, done)) return rc;
    au_halves_kernel<HID, D><<<std::min(a.n_tiles[0] + a.n_tiles[1], AU_GRID), FR_THREADS, lds, st>>>(a);
    AMID_LAUNCH_CHECK();
    return AMID_OK;
}

template <int HID>
static int au_topk_launch(const AuArgs& a, hipStream_t st) {
    const int per_wg = FR_THREADS >> 3;
    au_query_kernel<HID><<<(a.Q * HID + per_wg - 1) / per_wg, FR_THREADS, 0, st>>>(a);
    AMID_LAUNCH_CHECK();
    au_topk_kernel<HID><<<dim3(au_qgroups(a.Q), a.n_ranges), FR_THREADS, au_topk_lds_bytes(a.K), st>>>(a);
    AMID_LAUNCH_CHECK();
    au_merge_kernel<<<a.Q, FR_THREADS, fr_merge_lds_bytes(a.K), st>>>(a);
    AMID_LAUNCH_CHECK();
    return AMID_OK;
}

}  // namespace amid

using namespace amid;

extern "C" long long amid_audience_workspace_bytes(int Q, int n_d1, int n_d2, int hid, int k) {
    if (!au_sizes_ok(Q, n_d1, n_d2, k) || (hid != 16 && hid != 32 && hid != 64)) return -1;
    return au_workspace(Q, n_d1, n_d2, hid, k, nullptr, nullptr, nullptr);
}

extern "C" int amid_audience_target_workgroups(int wgs) {
    const int before = au_target_wgs;
    au_target_wgs = wgs >= 1 ? std::min(wgs, AU_TOPK_WGS) : AU_TOPK_WGS;
    return before;
}

extern "C" int amid_audience_halves_f32(const float* vectors, long long n_vectors, const int* slots_d1, int n_d1, const int* slots_d2, int n_d2,
                                        const float* w1, const float* b1, int D, int hid, void* workspace, int* flags, void* stream) {
    AMID_CHECK_ARG(vectors && w1 && b1 && workspace && flags);
    AMID_CHECK_ARG(au_sizes_ok(1, n_d1, n_d2, 1) && n_vectors >= 1 && n_vectors < 0x7fffffffLL);
    AMID_CHECK_ARG((slots_d1 != nullptr || n_d1 == 0) && (slots_d2 != nullptr || n_d2 == 0));
    if (!au_shape_ok(D, hid)) return AMID_ERR_UNSUPPORTED;
    AuArgs a{};
    a.v = vectors; a.n_vectors = n_vectors;
    a.slots[0] = slots_d1; a.slots[1] = slots_d2; a.n[0] = n_d1; a.n[1] = n_d2;
    a.n_tiles[0] = au_tiles(n_d1); a.n_tiles[1] = au_tiles(n_d2);
    a.w1 = w1; a.b1 = b1; a.D = D; a.hid = hid; a.flags = flags;
    a.uh = (float*)workspace;
    const hipStream_t st = (hipStream_t)stream;
    if (D == 64) return hid == 16 ? au_halves_launch<16, 64>(a, st) : hid == 32 ? au_halves_launch<32, 64>(a, st) : au_halves_launch<64, 64>(a, st);
    return hid == 16 ? au_halves_launch<16, 128>(a, st) : hid == 32 ? au_halves_launch<32, 128>(a, st) : au_halves_launch<64, 128>(a, st);
}

extern "C" int amid_audience_topk_f32(const long long* items, const long long* item_domain, int Q, const float* table, long long n_rows,
                                      const float* w1, const float* w2, const float* b2, const int* slots_d1, int n_d1, const int* slots_d2,
                                      int n_d2, const int* holders, const long long* holders_off, int D, int hid, int k, void* workspace,
                                      int* flags, long long* rows, float* scores, void* stream) {
    AMID_CHECK_ARG(items && item_domain && table && w1 && w2 && b2 && workspace && flags && rows && scores);
    AMID_CHECK_ARG(au_sizes_ok(Q, n_d1, n_d2, k) && n_rows >= 1 && n_rows <= 0x7fffffffLL);
    AMID_CHECK_ARG((slots_d1 != nullptr || n_d1 == 0) && (slots_d2 != nullptr || n_d2 == 0));
    AMID_CHECK_ARG(holders == nullptr || holders_off != nullptr);
    if (!au_shape_ok(D, hid)) return AMID_ERR_UNSUPPORTED;
    AuArgs a{};
    a.items = items; a.item_dom = item_domain; a.Q = Q; a.table = table; a.n_rows = n_rows;
    a.slots[0] = slots_d1; a.slots[1] = slots_d2; a.n[0] = n_d1; a.n[1] = n_d2;
    a.n_tiles[0] = au_tiles(n_d1); a.n_tiles[1] = au_tiles(n_d2);
    a.w1 = w1; a.w2 = w2; a.b2 = b2; a.hold = holders; a.hold_off = holders_off;
    a.D = D; a.hid = hid; a.K = k; a.flags = flags; a.out_rows = rows; a.out_s = scores;
    a.n_ranges = au_ranges(Q, a.n_tiles[0] + a.n_tiles[1]);
    size_t o_qh = 0, o_ps = 0, o_pi = 0;
    au_workspace(Q, n_d1, n_d2, hid, k, &o_qh, &o_ps, &o_pi);
    char* ws = (char*)workspace;
    a.uh = (float*)ws; a.qh = (float*)(ws + o_qh); a.part_s = (float*)(ws + o_ps); a.part_i = (int*)(ws + o_pi);
    const hipStream_t st = (hipStream_t)stream;
    return hid == 16 ? au_topk_launch<16>(a, st) : hid == 32 ? au_topk_launch<32>(a, st) : au_topk_launch<64>(a, st);
}
