// Full-catalog evaluation and top-K recommendation: B users scored against every candidate of their domain's item pool through
// predictModule (reference model_seq.py:32-54), p(u, c) = sigmoid(w2 . relu(W1[:, :D] u + b1 + W1[:, D:] E[c]) + b2).
//
// Over a shared catalog the item half W1[:, D:] E[c] does not depend on the user: it is formed ONCE per candidate, and per (user, candidate)
// pair only hid (add, max, fma) and the logit's tree remain.  Every piece is head_parts.h's (user_half_chain / item_half_chain joined by
// group_sum<8>, head_logit_p): p is bit-identical to what amid_eval_head_f32 / amid_head_fwd_f32 give for the same user vector and row.
//
// Launches (all on the caller's stream, no host synchronisation):
//   fr_user_kernel    a workgroup per user: au[b] = W1[:, :D] u_b + b1 into the workspace; with `pos`, the positive's score p0, the
//                     thresholds p0 - fix_value / p0, and rank[b] = -#{own items in the pool above them} (the count below includes them)
//   fr_count_kernel   persistent workgroups over tiles of FR_TILE pool candidates: the tile's item halves into LDS (eight lanes an output, the
//                     heads' chains), then a thread per candidate streams every user of the tile's domain past it; per-user counts of the
//                     candidates above the thresholds collect in LDS and are added to rank / rank_raw once per workgroup (integer atomics:
//                     any order, same sum)
//   fr_items_kernel   (top-K) the item halves of every pool candidate into the workspace
//   fr_topk_kernel    (top-K) a workgroup per (group of FR_UB users, range of tiles): a running best-K list per user in LDS; a tile's candidates
//                     that beat a list's K-th entry are merged into it by a bitonic sort of (list + newcomers)
//   fr_merge_kernel   (top-K) a workgroup per user: the ranges' lists through the same merge -> ids [B, K], scores [B, K]
// The history exclusion own(b) (sorted unique ids, at most a sequence long) is applied where its ids fall: the rank subtracts the own items'
// share of the count once per user, the top-K marks the own ids of a tile inside that tile.  No (user, candidate) pair is tested against
// the list.
#include <algorithm>
#include "head_parts.h"
#include "topk_list.h"

namespace amid {

#pragma clang fp contract(off)

constexpr int FR_TILE = 256;            // candidates per tile: one per thread
constexpr int FR_UCH = 1024;            // users per count launch (LDS counters)
constexpr int FR_UB = 8;                // users per top-K workgroup
constexpr int FR_GRID = 512;            // persistent workgroups of the count / item-half launches
constexpr int FR_TOPK_WGS = 1024;       // target workgroups of the top-K launch

struct FrArgs {
    const float* u; long long u_dom_stride;     // user b's vector: u + domain(b) * u_dom_stride + b * D
    const long long* pos;                       // [B] or null (top-K)
    const long long* domain;                    // [B]
    const long long* pool[2]; int n_pool[2];    // sorted unique candidate ids of each domain
    int n_tiles[2];
    const long long* own; const int* own_off; const int* rows;   // own(b) = own[own_off[rows[b]] .. own_off[rows[b] + 1]), or own null
    const float* table; long long n_rows;
    const float* w1; const float* b1; const float* w2; const float* b2;
    int B, D, hid, K, exclude;
    float fix_value;
    int* flags;
    float* au;                                  // workspace [B][hid]
    float* thr;                                 // workspace [B][2]
    float* ci;                                  // workspace [n_pool0 + n_pool1][hid] (top-K)
    float* part_s; int* part_i; int n_ranges;   // workspace [n_ranges][B][K] (top-K)
    int* rank; int* rank_raw;
    float* scores; long long n_cols;            // [B][n_cols] or null (rank)
    long long* out_ids; float* out_s;           // [B][K] (top-K)
    int u0, u1;                                 // users of this count launch
};

__device__ __forceinline__ int fr_dom(const FrArgs& a, int b) { return a.domain[b] != 0 ? 1 : 0; }
__device__ __forceinline__ bool fr_id_ok(const FrArgs& a, long long id) { return id >= 0 && id < a.n_rows; }

__device__ __forceinline__ bool fr_in_pool(const long long* pool, int n, long long id) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (pool[mid] < id) lo = mid + 1; else hi = mid;
    }
    return lo < n && pool[lo] == id;
}

// ---- per user: au, thresholds, the own items' share of the count ----------------------------------------------------------------------------
template <int HID>
__global__ __launch_bounds__(FR_THREADS) void fr_user_kernel(const FrArgs a) {
    __shared__ float au_s[HID], ci_s[HID];
    __shared__ float thr_s[2];
    const int b = blockIdx.x, D = a.D, tid = threadIdx.x, part = tid & 7;
    const int dom = fr_dom(a, b);
    const float* ub = a.u + dom * a.u_dom_stride + (long long)b * D;
    for (int o0 = 0; o0 < HID; o0 += FR_THREADS >> 3) {                  // (uniform trip count: the shuffles need every lane)
        const int j = o0 + (tid >> 3);
        const bool on = j < HID;
        float acc = on ? user_half_chain(a.w1 + (long long)j * 2 * D, 1, ub, D, part) : 0.f;
        acc = group_sum<8>(acc);
        if (on && part == 0) {
            au_s[j] = acc + a.b1[j];
            a.au[(long long)b * HID + j] = acc + a.b1[j];
        }
    }
    if (a.pos == nullptr) return;
    __syncthreads();
    // item 0: the positive; items 1..: the own ids that are candidates (members of the pool)
    int lo = 0, n_own = 0;
    if (a.own != nullptr) { const int r = a.rows[b]; lo = a.own_off[r]; n_own = a.own_off[r + 1] - lo; }
    int ex = 0, ex_raw = 0;
    for (int i = 0; i <= n_own; ++i) {                         // (uniform: every thread looks at the same id)
        const long long id = i == 0 ? a.pos[b] : a.own[lo + i - 1];
        if (!fr_id_ok(a, id)) {
            if (tid == 0) {
                atomicOr(a.flags, AMID_FLAG_INDEX_RANGE);
                if (i == 0) { thr_s[0] = __builtin_nanf(""); thr_s[1] = __builtin_nanf(""); }
            }
            continue;
        }
        if (i > 0 && !fr_in_pool(a.pool[dom], a.n_pool[dom], id)) continue;
        const float* row = a.table + id * D;
        for (int o0 = 0; o0 < HID; o0 += FR_THREADS >> 3) {
            const int j = o0 + (tid >> 3);
            const bool on = j < HID;
            float acc = on ? item_half_chain(a.w1 + (long long)j * 2 * D + D, 1, row, D, part) : 0.f;
            acc = group_sum<8>(acc);
            if (on && part == 0) ci_s[j] = acc;
        }
        __syncthreads();
        if (tid == 0) {
            const float p = head_logit_p<HID>([&](int j) { return au_s[j]; }, [&](int j) { return ci_s[j]; }, a.w2, a.b2[0]);
            if (i == 0) { thr_s[0] = p - a.fix_value; thr_s[1] = p; }
            else { ex += p > thr_s[0] ? 1 : 0; ex_raw += p > thr_s[1] ? 1 : 0; }
        }
        __syncthreads();
    }
    if (tid == 0) {
        a.thr[2 * b] = thr_s[0]; a.thr[2 * b + 1] = thr_s[1];
        a.rank[b] = -ex; a.rank_raw[b] = -ex_raw;
    }
}

// W1[:, D:]^T -> w1t [D][HID + 1]
template <int HID>
__device__ __forceinline__ void fr_stage_w1t(const FrArgs& a, float* __restrict__ w1t) {
    const int D = a.D;
    for (int x = threadIdx.x; x < HID * D; x += FR_THREADS) {
        const int j = x / D, e = x - j * D;
        w1t[e * (HID + 1) + j] = a.w1[(long long)j * 2 * D + D + e];
    }
}

// item halves of candidates n0 .. n0 + nn - 1 of pool `dom` into out[n * ld + j] (item_half's eight lanes an output); w1t: fr_stage_w1t's.
// Ids outside the table raise the index flag and read row 0 (their scores are never used).
template <int HID>
__device__ __forceinline__ void fr_tile_item_halves(const FrArgs& a, const float* __restrict__ w1t, int dom, int n0, int nn, float* out, int ld) {
    const int D = a.D, tid = threadIdx.x, part = tid & 7;
    const long long* pool = a.pool[dom];
    for (int o0 = 0; o0 < nn * HID; o0 += FR_THREADS >> 3) {           // (uniform trip count)
        const int nj = o0 + (tid >> 3);
        const int n = nj / HID, j = nj - n * HID;
        const bool on = n < nn;
        float acc = 0.f;
        if (on) {
            long long id = pool[n0 + n];
            if (!fr_id_ok(a, id)) {
                if (part == 0 && j == 0) atomicOr(a.flags, AMID_FLAG_INDEX_RANGE);
                id = 0;
            }
            acc = item_half_chain(w1t + j, HID + 1, a.table + id * D, D, part);
        }
        acc = group_sum<8>(acc);
        if (on && part == 0) out[(long long)n * ld + j] = acc;
    }
}

__device__ __forceinline__ void fr_tile_of(const FrArgs& a, int t, int& dom, int& n0, int& nn) {
    dom = t < a.n_tiles[0] ? 0 : 1;
    n0 = (dom ? t - a.n_tiles[0] : t) * FR_TILE;
    nn = min(FR_TILE, a.n_pool[dom] - n0);
}

// ---- rank: counts of the candidates above each user's thresholds ------------------------------------------------------------------------------
template <int HID>
__global__ __launch_bounds__(FR_THREADS) void fr_count_kernel(const FrArgs a) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float* w1t = sm;                                                   // [D][HID + 1]
    float* ci_s = w1t + a.D * (HID + 1);                               // [FR_TILE][HID + 1]
    int* cnt = reinterpret_cast<int*>(ci_s + FR_TILE * (HID + 1));     // [FR_UCH][2]
    const int tid = threadIdx.x, nu = a.u1 - a.u0;
    fr_stage_w1t<HID>(a, w1t);
    for (int i = tid; i < 2 * nu; i += FR_THREADS) cnt[i] = 0;
    const int n_t = a.n_tiles[0] + a.n_tiles[1];
    for (int t = blockIdx.x; t < n_t; t += gridDim.x) {
        int dom, n0, nn;
        fr_tile_of(a, t, dom, n0, nn);
        __syncthreads();                                               // (w1t staged; the previous tile's item halves read)
        fr_tile_item_halves<HID>(a, w1t, dom, n0, nn, ci_s, HID + 1);
        __syncthreads();
        const bool on = tid < nn;
        const long long id = on ? a.pool[dom][n0 + tid] : -1;
        const bool valid = on && fr_id_ok(a, id);
        float c[HID];
#pragma unroll
        for (int j = 0; j < HID; ++j) c[j] = ci_s[tid * (HID + 1) + j];
        for (int b = a.u0; b < a.u1; ++b) {
            if (fr_dom(a, b) != dom) continue;                         // (uniform)
            const float* aub = a.au + (long long)b * HID;
            const float p = head_logit_p<HID>([&](int j) { return aub[j]; }, [&](int j) { return c[j]; }, a.w2, a.b2[0]);
            const float th = a.thr[2 * b], th_raw = a.thr[2 * b + 1];
            const int k1 = __popcll(__ballot(valid && p > th)), k2 = __popcll(__ballot(valid && p > th_raw));
            if (lane_id() == 0 && (k1 | k2)) { atomicAdd(&cnt[2 * (b - a.u0)], k1); atomicAdd(&cnt[2 * (b - a.u0) + 1], k2); }
            if (a.scores != nullptr && on) a.scores[(long long)b * a.n_cols + n0 + tid] = valid ? p : __builtin_nanf("");
        }
    }
    __syncthreads();
    for (int i = tid; i < nu; i += FR_THREADS) {
        const int k1 = cnt[2 * i], k2 = cnt[2 * i + 1];
        if (k1) atomicAdd(&a.rank[a.u0 + i], k1);
        if (k2) atomicAdd(&a.rank_raw[a.u0 + i], k2);
    }
}

// ---- top-K ----------------------------------------------------------------------------------------------------------------------------------
template <int HID>
__global__ __launch_bounds__(FR_THREADS) void fr_items_kernel(const FrArgs a) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float* w1t = sm;
    fr_stage_w1t<HID>(a, w1t);
    __syncthreads();
    const int n_t = a.n_tiles[0] + a.n_tiles[1];
    for (int t = blockIdx.x; t < n_t; t += gridDim.x) {
        int dom, n0, nn;
        fr_tile_of(a, t, dom, n0, nn);
        fr_tile_item_halves<HID>(a, w1t, dom, n0, nn, a.ci + ((long long)(dom ? a.n_pool[0] : 0) + n0) * HID, HID);
    }
}


// LDS (4-byte words): lists [FR_UB][K] scores | [FR_UB][K] ids | n [FR_UB] | merge [512] scores | [512] ids | wcnt [4] | ex [FR_TILE] |
// tile ids [FR_TILE] (8-byte)
__host__ __device__ inline size_t fr_topk_lds_bytes(int K) {
    return (size_t)4 * (2 * FR_UB * K + FR_UB + 2 * 512 + 4 + FR_TILE) + 8 * FR_TILE;
}

template <int HID>
__global__ __launch_bounds__(FR_THREADS) void fr_topk_kernel(const FrArgs a) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int K = a.K, tid = threadIdx.x;
    float* ls = sm;
    int* li = reinterpret_cast<int*>(ls + FR_UB * K);
    int* ln = li + FR_UB * K;
    FrScratch S;
    S.s = reinterpret_cast<float*>(ln + FR_UB);
    S.id = reinterpret_cast<int*>(S.s + 512);
    S.wcnt = S.id + 512;
    int* ex = S.wcnt + 4;
    long long* ids_s = reinterpret_cast<long long*>(ex + FR_TILE);     // (8-byte aligned: every count in front of it is even)
    const int b0 = blockIdx.x * FR_UB, nb = min(FR_UB, a.B - b0);
    const int r = blockIdx.y;
    const int n_t = a.n_tiles[0] + a.n_tiles[1];
    const int per = (n_t + a.n_ranges - 1) / a.n_ranges;
    const int t0 = r * per, t1 = min(n_t, t0 + per);
    if (tid < FR_UB) ln[tid] = 0;
    for (int t = t0; t < t1; ++t) {
        int dom, n0, nn;
        fr_tile_of(a, t, dom, n0, nn);
        const bool on = tid < nn;
        const long long id = on ? a.pool[dom][n0 + tid] : -1;
        const bool valid = on && fr_id_ok(a, id);
        __syncthreads();                                               // (the previous tile's searches of ids_s are done)
        ids_s[tid] = id;
        float c[HID];
        const float* cr = a.ci + ((long long)(dom ? a.n_pool[0] : 0) + n0 + (on ? tid : 0)) * HID;
#pragma unroll
        for (int j = 0; j < HID; ++j) c[j] = cr[j];
        for (int i = 0; i < nb; ++i) {
            const int b = b0 + i;
            if (fr_dom(a, b) != dom) continue;                         // (uniform)
            ex[tid] = 0;
            __syncthreads();                                           // (ids_s and ex written; the previous user's offer has read ex)
            if (a.exclude && a.own != nullptr) {
                const int rr = a.rows[b], lo = a.own_off[rr], hi = a.own_off[rr + 1];
                const long long first = ids_s[0], last = ids_s[nn - 1];
                for (int k = lo + tid; k < hi; k += FR_THREADS) {
                    const long long o = a.own[k];
                    if (o < first || o > last) continue;
                    int l = 0, h = nn;
                    while (l < h) { const int mid = (l + h) >> 1; if (ids_s[mid] < o) l = mid + 1; else h = mid; }
                    if (l < nn && ids_s[l] == o) ex[l] = 1;
                }
                __syncthreads();
            }
            const float* aub = a.au + (long long)b * HID;
            const float p = head_logit_p<HID>([&](int j) { return aub[j]; }, [&](int j) { return c[j]; }, a.w2, a.b2[0]);
            const FrList L{ls + i * K, li + i * K, ln + i};
            fr_offer(L, S, K, valid && ex[tid] == 0, p, (int)id);
        }
    }
    __syncthreads();
    for (int i = 0; i < nb; ++i) {
        const int n = ln[i];
        const long long o = ((long long)r * a.B + b0 + i) * K;
        for (int k = tid; k < K; k += FR_THREADS) {
            a.part_s[o + k] = k < n ? ls[i * K + k] : -INFINITY;
            a.part_i[o + k] = k < n ? li[i * K + k] : FR_ID_NONE;
        }
    }
}

__global__ __launch_bounds__(FR_THREADS) void fr_merge_kernel(const FrArgs a) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    fr_merge_ranges(sm, a.K, a.n_ranges, a.B, blockIdx.x, a.part_s, a.part_i, a.out_ids, a.out_s);
}

#pragma clang fp contract(fast)

// ---- host side ------------------------------------------------------------------------------------------------------------------------------
static inline int fr_tiles(int n) { return (n + FR_TILE - 1) / FR_TILE; }
static inline int fr_ranges(int B, int n_tiles) {
    const int n_uc = (B + FR_UB - 1) / FR_UB;
    return std::max(1, std::min(n_tiles, (FR_TOPK_WGS + n_uc - 1) / n_uc));
}
static inline size_t fr_align(size_t x) { return (x + 255) & ~(size_t)255; }

// workspace carve: au [B][hid] | thr [B][2] | (top-K) ci [n1 + n2][hid] | part_s [R][B][K] | part_i [R][B][K]
static long long fr_workspace(int B, int n1, int n2, int hid, int k, size_t* off_thr, size_t* off_ci, size_t* off_ps, size_t* off_pi) {
    size_t o = fr_align((size_t)B * hid * 4);
    if (off_thr) *off_thr = o;
    o += fr_align((size_t)B * 2 * 4);
    if (k > 0) {
        if (off_ci) *off_ci = o;
        o += fr_align(((size_t)n1 + n2) * hid * 4);
        const size_t part = (size_t)fr_ranges(B, fr_tiles(n1) + fr_tiles(n2)) * B * k * 4;
        if (off_ps) *off_ps = o;
        o += fr_align(part);
        if (off_pi) *off_pi = o;
        o += fr_align(part);
    }
    return (long long)o;
}

static bool fr_shape_ok(int D, int hid) { return (D == 64 || D == 128) && (hid == 16 || hid == 32 || hid == 64); }

static void fr_fill(FrArgs& a, const float* u, long long u_dom_stride, const long long* domain_id, int B, const long long* pool_d1, int n_pool_d1,
                    const long long* pool_d2, int n_pool_d2, const long long* own_items, const int* own_off, const int* rows, const float* table,
                    long long n_rows, const float* w1, const float* b1, const float* w2, const float* b2, int D, int hid, int k, void* workspace,
                    int* flags) {
    a = FrArgs{};
    a.u = u; a.u_dom_stride = u_dom_stride; a.domain = domain_id;
    a.pool[0] = pool_d1; a.pool[1] = pool_d2; a.n_pool[0] = n_pool_d1; a.n_pool[1] = n_pool_d2;
    a.n_tiles[0] = fr_tiles(n_pool_d1); a.n_tiles[1] = fr_tiles(n_pool_d2);
    a.own = own_items; a.own_off = own_off; a.rows = rows;
    a.table = table; a.n_rows = n_rows; a.w1 = w1; a.b1 = b1; a.w2 = w2; a.b2 = b2;
    a.B = B; a.D = D; a.hid = hid; a.K = k; a.flags = flags;
    size_t o_thr = 0, o_ci = 0, o_ps = 0, o_pi = 0;
    fr_workspace(B, n_pool_d1, n_pool_d2, hid, k, &o_thr, &o_ci, &o_ps, &o_pi);
    char* ws = (char*)workspace;
    a.au = (float*)ws; a.thr = (float*)(ws + o_thr);
    if (k > 0) {
        a.ci = (float*)(ws + o_ci); a.part_s = (float*)(ws + o_ps); a.part_i = (int*)(ws + o_pi);
        a.n_ranges = fr_ranges(B, a.n_tiles[0] + a.n_tiles[1]);
    }
}

template <int HID>
static int fr_rank_launch(FrArgs a, hipStream_t st) {
    static unsigned long long done = 0;
    fr_user_kernel<HID><<<a.B, FR_THREADS, 0, st>>>(a);
    AMID_LAUNCH_CHECK();
    const size_t lds = ((size_t)a.D * (HID + 1) + (size_t)FR_TILE * (HID + 1) + 2 * FR_UCH) * 4;
    if (int rc = lds_attr_once((const void*)fr_count_kernel<HID>, 160 * 1024, done)) return rc;
    const int n_t = a.n_tiles[0] + a.n_tiles[1];
    for (int u0 = 0; u0 < a.B; u0 += FR_UCH) {
        a.u0 = u0; a.u1 = std::min(a.B, u0 + FR_UCH);
        fr_count_kernel<HID><<<std::min(n_t, FR_GRID), FR_THREADS, lds, st>>>(a);
        AMID_LAUNCH_CHECK();
    }
    return AMID_OK;
}

template <int HID>
static int fr_topk_launch(FrArgs a, hipStream_t st) {
    static unsigned long long done_items = 0, done_topk = 0, done_merge = 0;
    fr_user_kernel<HID><<<a.B, FR_THREADS, 0, st>>>(a);
    AMID_LAUNCH_CHECK();
    const int n_t = a.n_tiles[0] + a.n_tiles[1];
    if (int rc = lds_attr_once((const void*)fr_items_kernel<HID>, 160 * 1024, done_items)) return rc;
    fr_items_kernel<HID><<<std::min(n_t, FR_GRID), FR_THREADS, (size_t)a.D * (HID + 1) * 4, st>>>(a);
    AMID_LAUNCH_CHECK();
    if (int rc = lds_attr_once((const void*)fr_topk_kernel<HID>, 160 * 1024, done_topk)) return rc;
    fr_topk_kernel<HID><<<dim3((a.B + FR_UB - 1) / FR_UB, a.n_ranges), FR_THREADS, fr_topk_lds_bytes(a.K), st>>>(a);
    AMID_LAUNCH_CHECK();
    if (int rc = lds_attr_once((const void*)fr_merge_kernel, 160 * 1024, done_merge)) return rc;
    fr_merge_kernel<<<a.B, FR_THREADS, fr_merge_lds_bytes(a.K), st>>>(a);
    AMID_LAUNCH_CHECK();
    return AMID_OK;
}

// fr_topk_launch cut where it stops depending on the user: the item halves alone (frozen weights: once for every batch of a dataset) ...
template <int HID>
static int fr_topk_items_launch(FrArgs a, hipStream_t st) {
    static unsigned long long done_items = 0;
    const int n_t = a.n_tiles[0] + a.n_tiles[1];
    if (int rc = lds_attr_once((const void*)fr_items_kernel<HID>, 160 * 1024, done_items)) return rc;
    fr_items_kernel<HID><<<std::min(n_t, FR_GRID), FR_THREADS, (size_t)a.D * (HID + 1) * 4, st>>>(a);
    AMID_LAUNCH_CHECK();
    return AMID_OK;
}

// ... and the rest, reading the ci region an earlier fr_topk_items_launch filled (the same kernels on the same operands as fr_topk_launch:
// fr_user_kernel and fr_items_kernel write disjoint regions and read nothing of each other)
template <int HID>
static int fr_topk_users_launch(FrArgs a, hipStream_t st) {
    static unsigned long long done_topk = 0, done_merge = 0;
    fr_user_kernel<HID><<<a.B, FR_THREADS, 0, st>>>(a);
    AMID_LAUNCH_CHECK();
    if (int rc = lds_attr_once((const void*)fr_topk_kernel<HID>, 160 * 1024, done_topk)) return rc;
    fr_topk_kernel<HID><<<dim3((a.B + FR_UB - 1) / FR_UB, a.n_ranges), FR_THREADS, fr_topk_lds_bytes(a.K), st>>>(a);
    AMID_LAUNCH_CHECK();
    if (int rc = lds_attr_once((const void*)fr_merge_kernel, 160 * 1024, done_merge)) return rc;
    fr_merge_kernel<<<a.B, FR_THREADS, fr_merge_lds_bytes(a.K), st>>>(a);
    AMID_LAUNCH_CHECK();
    return AMID_OK;
}

}  // namespace amid

using namespace amid;

extern "C" long long amid_full_rank_workspace_bytes(int B, int n_pool_d1, int n_pool_d2, int hid, int k) {
    if (B < 1 || n_pool_d1 < 1 || n_pool_d2 < 1 || hid < 1 || k < 0 || k > 256) return -1;
    return fr_workspace(B, n_pool_d1, n_pool_d2, hid, k, nullptr, nullptr, nullptr, nullptr);
}

extern "C" int amid_full_rank_f32(const float* u, long long u_dom_stride, const long long* pos, const long long* domain_id, int B,
                                  const long long* pool_d1, int n_pool_d1, const long long* pool_d2, int n_pool_d2, const long long* own_items,
                                  const int* own_off, const int* rows, const float* table, long long n_rows, const float* w1, const float* b1,
                                  const float* w2, const float* b2, int D, int hid, float fix_value, void* workspace, int* flags, int* rank,
                                  int* rank_raw, float* scores, long long n_cols, void* stream) {
    AMID_CHECK_ARG(u && pos && domain_id && pool_d1 && pool_d2 && table && w1 && b1 && w2 && b2 && workspace && flags && rank && rank_raw);
    AMID_CHECK_ARG(B >= 1 && n_pool_d1 >= 1 && n_pool_d2 >= 1 && n_rows >= 1 && n_rows <= 0x7fffffffLL && u_dom_stride >= 0);
    AMID_CHECK_ARG(own_items == nullptr || (own_off && rows));
    AMID_CHECK_ARG(scores == nullptr || n_cols >= (long long)std::max(n_pool_d1, n_pool_d2));
    if (!fr_shape_ok(D, hid)) return AMID_ERR_UNSUPPORTED;
    FrArgs a;
    fr_fill(a, u, u_dom_stride, domain_id, B, pool_d1, n_pool_d1, pool_d2, n_pool_d2, own_items, own_off, rows, table, n_rows, w1, b1, w2, b2,
            D, hid, 0, workspace, flags);
    a.pos = pos; a.fix_value = fix_value; a.rank = rank; a.rank_raw = rank_raw; a.scores = scores; a.n_cols = n_cols;
    const hipStream_t st = (hipStream_t)stream;
    return hid == 16 ? fr_rank_launch<16>(a, st) : hid == 32 ? fr_rank_launch<32>(a, st) : fr_rank_launch<64>(a, st);
}

extern "C" int amid_topk_f32(const float* u, long long u_dom_stride, const long long* domain_id, int B, const long long* pool_d1, int n_pool_d1,
                             const long long* pool_d2, int n_pool_d2, const long long* own_items, const int* own_off, const int* rows,
                             const float* table, long long n_rows, const float* w1, const float* b1, const float* w2, const float* b2, int D,
                             int hid, int k, int exclude_history, void* workspace, int* flags, long long* ids, float* scores, void* stream) {
    AMID_CHECK_ARG(u && domain_id && pool_d1 && pool_d2 && table && w1 && b1 && w2 && b2 && workspace && flags && ids && scores);
    AMID_CHECK_ARG(k >= 1 && k <= 256);
    AMID_CHECK_ARG(B >= 1 && n_pool_d1 >= 1 && n_pool_d2 >= 1 && n_rows >= 1 && n_rows <= 0x7fffffffLL && u_dom_stride >= 0);
    AMID_CHECK_ARG(!exclude_history || own_items == nullptr || (own_off && rows));
    if (!fr_shape_ok(D, hid)) return AMID_ERR_UNSUPPORTED;
    FrArgs a;
    fr_fill(a, u, u_dom_stride, domain_id, B, pool_d1, n_pool_d1, pool_d2, n_pool_d2, exclude_history ? own_items : nullptr, own_off, rows,
            table, n_rows, w1, b1, w2, b2, D, hid, k, workspace, flags);
    a.exclude = exclude_history ? 1 : 0; a.out_ids = ids; a.out_s = scores;
    const hipStream_t st = (hipStream_t)stream;
    return hid == 16 ? fr_topk_launch<16>(a, st) : hid == 32 ? fr_topk_launch<32>(a, st) : fr_topk_launch<64>(a, st);
}

// amid_topk_f32 as two calls (a dataset's batches against frozen weights: the item halves once, the rest per batch).  Both carve the
// workspace as amid_topk_f32 does for (B, n_pool_d1, n_pool_d2, hid, k >= 1); where the ci region starts depends on B and hid only.
extern "C" int amid_topk_items_f32(int B, const long long* pool_d1, int n_pool_d1, const long long* pool_d2, int n_pool_d2, const float* table,
                                   long long n_rows, const float* w1, int D, int hid, void* workspace, int* flags, void* stream) {
    AMID_CHECK_ARG(pool_d1 && pool_d2 && table && w1 && workspace && flags);
    AMID_CHECK_ARG(B >= 1 && n_pool_d1 >= 1 && n_pool_d2 >= 1 && n_rows >= 1 && n_rows <= 0x7fffffffLL);
    if (!fr_shape_ok(D, hid)) return AMID_ERR_UNSUPPORTED;
    FrArgs a;
    fr_fill(a, nullptr, 0, nullptr, B, pool_d1, n_pool_d1, pool_d2, n_pool_d2, nullptr, nullptr, nullptr, table, n_rows, w1, nullptr, nullptr,
            nullptr, D, hid, 1, workspace, flags);
    const hipStream_t st = (hipStream_t)stream;
    return hid == 16 ? fr_topk_items_launch<16>(a, st) : hid == 32 ? fr_topk_items_launch<32>(a, st) : fr_topk_items_launch<64>(a, st);
}

extern "C" int amid_topk_users_f32(const float* u, long long u_dom_stride, const long long* domain_id, int B, const long long* pool_d1,
                                   int n_pool_d1, const long long* pool_d2, int n_pool_d2, const long long* own_items, const int* own_off,
                                   const int* rows, const float* table, long long n_rows, const float* w1, const float* b1, const float* w2,
                                   const float* b2, int D, int hid, int k, int exclude_history, void* workspace, int* flags, long long* ids,
                                   float* scores, void* stream) {
    AMID_CHECK_ARG(u && domain_id && pool_d1 && pool_d2 && table && w1 && b1 && w2 && b2 && workspace && flags && ids && scores);
    AMID_CHECK_ARG(k >= 1 && k <= 256);
    AMID_CHECK_ARG(B >= 1 && n_pool_d1 >= 1 && n_pool_d2 >= 1 && n_rows >= 1 && n_rows <= 0x7fffffffLL && u_dom_stride >= 0);
    AMID_CHECK_ARG(!exclude_history || own_items == nullptr || (own_off && rows));
    if (!fr_shape_ok(D, hid)) return AMID_ERR_UNSUPPORTED;
    FrArgs a;
    fr_fill(a, u, u_dom_stride, domain_id, B, pool_d1, n_pool_d1, pool_d2, n_pool_d2, exclude_history ? own_items : nullptr, own_off, rows,
            table, n_rows, w1, b1, w2, b2, D, hid, k, workspace, flags);
    a.exclude = exclude_history ? 1 : 0; a.out_ids = ids; a.out_s = scores;
    const hipStream_t st = (hipStream_t)stream;
    return hid == 16 ? fr_topk_users_launch<16>(a, st) : hid == 32 ? fr_topk_users_launch<32>(a, st) : fr_topk_users_launch<64>(a, st);
}
