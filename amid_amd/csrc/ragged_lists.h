// Ragged per-row lists on the device, as rank_lists.hip and diversify.hip walk them: row b owns cand[cand_off[b] .. cand_off[b + 1]), the
// offsets clamped into [0, n_cand] on the device, and the host never reads one.  A list is cut into tiles of RL_TILE entries and a row's
// tiles into UNITS of `per` consecutive tiles (per = ceil(tile bound / target workgroups), from the host's n_cand and B alone); a unit
// keeps a running best-K list, and a row's units' lists go through the same merge.
//
// The best-K list is topk_list.h's in shape (a list in LDS, newcomers merged by a bitonic sort of list + newcomers, the merges deferred as
// audience.hip's au_offer defers them) with a 64-bit key in place of the int id: (id << 32) | position.  The order -- larger score first,
// ties to the lower id, further ties to the lower position -- is total over a list's entries, so the k best and their order do not depend
// on how the list was cut into tiles and units or on which workgroup took which unit.
#pragma once
#include <algorithm>
#include "topk_list.h"
#include "amid_hip.h"

namespace amid {

constexpr int RL_TILE = 256;            // entries per tile: one per thread of the offer
constexpr int RL_PEND = 256;            // newcomers a list collects between two merges (list + pending <= the 512 of the merge buffer)
constexpr int RL_GRID = 1024;           // persistent workgroups of a launch over the units at most
constexpr int RL_UNITS = 2048;          // target number of units at most
constexpr unsigned long long RL_KEY_NONE = ~0ull;       // an empty list slot (sorts after every entry)

// ---- the list: topk_list.h's, keyed by (id << 32) | position ------------------------------------------------------------------------------------
__device__ __forceinline__ bool rl_before(float s1, unsigned long long k1, float s2, unsigned long long k2) {
    return s1 > s2 || (s1 == s2 && k1 < k2);
}
struct RlList { float* s; unsigned long long* key; int* n; };          // the running best-K list
struct RlScratch { float* s; unsigned long long* key; int* wcnt; };     // merge buffer [512]; per-wave counts [4]
struct RlPending { float* s; unsigned long long* key; int* n; };        // [RL_PEND]
struct RlLds { RlList L; RlScratch S; RlPending P; float* rest; };

// LDS of a list: keys [Kp] | merge keys [512] | pending keys [RL_PEND] | scores [Kp] | merge scores [512] | pending scores [RL_PEND] |
// n, pending n, wcnt [4], 2 spare  (Kp = K rounded up to a multiple of 4: 12 Kp bytes, so everything behind stays 16-byte aligned)
__host__ __device__ inline size_t rl_list_lds_bytes(int K) {
    const size_t Kp = (size_t)(K + 3) & ~(size_t)3;
    return 8 * (Kp + 512 + RL_PEND) + 4 * (Kp + 512 + RL_PEND) + 4 * 8;
}
__device__ __forceinline__ RlLds rl_carve(void* sm, int K) {
    const int Kp = (K + 3) & ~3;
    RlLds c;
    c.L.key = reinterpret_cast<unsigned long long*>(sm);
    c.S.key = c.L.key + Kp;
    c.P.key = c.S.key + 512;
    c.L.s = reinterpret_cast<float*>(c.P.key + RL_PEND);
    c.S.s = c.L.s + Kp;
    c.P.s = c.S.s + 512;
    c.L.n = reinterpret_cast<int*>(c.P.s + RL_PEND);
    c.P.n = c.L.n + 1;
    c.S.wcnt = c.L.n + 2;
    c.rest = reinterpret_cast<float*>(c.L.n + 8);
    return c;
}

// fr_sort_keep with the 64-bit key: the list's n entries to the front of the merge buffer, whose entries [n, total) the caller has written;
// bitonic sort, best first; the first min(K, total) become the list.  Every thread of the workgroup calls this; it ends in a barrier.
__device__ __forceinline__ void rl_sort_keep(const RlList& L, const RlScratch& S, int K, int n, int total) {
    const int tid = threadIdx.x;
    int size = 2;
    while (size < total) size <<= 1;
    for (int i = tid; i < size; i += FR_THREADS) {
        if (i < n) { S.s[i] = L.s[i]; S.key[i] = L.key[i]; }
        else if (i >= total) { S.s[i] = -INFINITY; S.key[i] = RL_KEY_NONE; }
    }
    __syncthreads();
    for (int k = 2; k <= size; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < (size >> 1); t += FR_THREADS) {
                const int i = 2 * j * (t / j) + (t % j), l = i + j;
                const float sa = S.s[i], sb = S.s[l];
                const unsigned long long ka = S.key[i], kb = S.key[l];
                const bool first = (i & k) == 0;               // this run ends up best-first
                if (first ? rl_before(sb, kb, sa, ka) : rl_before(sa, ka, sb, kb)) {
                    S.s[i] = sb; S.s[l] = sa; S.key[i] = kb; S.key[l] = ka;
                }
            }
            __syncthreads();
        }
    }
    const int keep = min(K, total);
    for (int i = tid; i < keep; i += FR_THREADS) { L.s[i] = S.s[i]; L.key[i] = S.key[i]; }
    if (tid == 0) *L.n = keep;
    __syncthreads();
}

// merge the pn pending newcomers into the list (every thread of the workgroup; pn uniform)
__device__ __forceinline__ void rl_flush(const RlLds& c, int K, int pn) {
    __syncthreads();                                                   // (the pending entries are written)
    const int n = *c.L.n;
    for (int x = threadIdx.x; x < pn; x += FR_THREADS) { c.S.s[n + x] = c.P.s[x]; c.S.key[n + x] = c.P.key[x]; }
    if (threadIdx.x == 0) *c.P.n = 0;
    rl_sort_keep(c.L, c.S, K, n, n + pn);                              // (n + pn <= K + RL_PEND <= 512)
}

// Offer one entry per thread (cand: it takes part); every thread of the workgroup calls this.  au_offer's form: newcomers that beat the
// list's K-th entry AS IT STANDS collect in the pending buffer and are merged only when the next call's might not fit (and by the caller
// at the end).  The K-th entry only rises at a merge, so the test lets through a superset of what a fresh list would: the k best and
// their order are the same.  A list that is not full yet merges at once.  Every path that writes the list or the pending count ends in a
// barrier, so two calls on one list may follow each other directly.
__device__ __forceinline__ void rl_offer(const RlLds& c, int K, bool cand, float s, unsigned long long key) {
    const int tid = threadIdx.x, lane = lane_id(), w = tid >> 6;
    const int n = *c.L.n;
    int pn = *c.P.n;
    bool beat = cand;
    if (cand && n == K) beat = rl_before(s, key, c.L.s[K - 1], c.L.key[K - 1]);
    const unsigned long long m = __ballot(beat);
    if (lane == 0) c.S.wcnt[w] = __popcll(m);
    __syncthreads();
    int off = 0, tot = 0;
    for (int v = 0; v < FR_THREADS / 64; ++v) { off += v < w ? c.S.wcnt[v] : 0; tot += c.S.wcnt[v]; }
    __syncthreads();                                           // (every wave has read the counts, n and pn before anything below writes them)
    if (tot == 0) return;                                      // (uniform)
    if (pn + tot > RL_PEND) { rl_flush(c, K, pn); pn = 0; }    // (uniform; the newcomers were tested against the older, lower K-th entry)
    if (beat) {
        const int slot = pn + off + __popcll(m & ((1ull << lane) - 1ull));
        c.P.s[slot] = s; c.P.key[slot] = key;
    }
    if (n < K) rl_flush(c, K, pn + tot);                       // (pn is 0 here: a list that is not full never leaves anything pending)
    else {
        if (tid == 0) *c.P.n = pn + tot;
        __syncthreads();                                       // (the next call, or the caller's last flush, reads the pending count at once)
    }
}

__device__ __forceinline__ void rl_list_reset(const RlLds& c) {
    __syncthreads();                                           // (the previous list is read)
    if (threadIdx.x == 0) { *c.L.n = 0; *c.P.n = 0; }
    __syncthreads();
}

// what is still pending goes in; the slots behind the list's last entry become empty ones.  Every thread of the workgroup; ends in a barrier.
__device__ __forceinline__ void rl_list_close(const RlLds& c, int K) {
    __syncthreads();
    const int pn = *c.P.n;
    if (pn > 0) rl_flush(c, K, pn);                            // (uniform)
    for (int k = *c.L.n + threadIdx.x; k < K; k += FR_THREADS) { c.L.s[k] = -INFINITY; c.L.key[k] = RL_KEY_NONE; }
    __syncthreads();
}

// nu > 1 lists of K slots each, ps / pk [nu][K] (empty slots: RL_KEY_NONE), merged into the list of c, closed (rl_list_close)
__device__ __forceinline__ void rl_merge_units(const RlLds& c, int K, const float* ps, const unsigned long long* pk, int nu) {
    const int tid = threadIdx.x;
    rl_list_reset(c);
    const long long E = (long long)nu * K;
    unsigned long long key_next = tid < E ? pk[tid] : RL_KEY_NONE;
    float s_next = tid < E ? ps[tid] : -INFINITY;
    for (long long e0 = 0; e0 < E; e0 += FR_THREADS) {         // (the next entries' loads are in flight behind the offer's barriers)
        const unsigned long long key = key_next;
        const float s = s_next;
        const long long e = e0 + FR_THREADS + tid;
        key_next = e < E ? pk[e] : RL_KEY_NONE;
        s_next = e < E ? ps[e] : -INFINITY;
        rl_offer(c, K, key != RL_KEY_NONE, s, key);
    }
    rl_list_close(c, K);
}

// ---- rows, tiles, units -------------------------------------------------------------------------------------------------------------------------
// row b's list [lo, lo + len) with both offsets clamped into [0, n_cand]; an offset outside, or a falling pair (an empty list), raises the
// flag (flags null: nothing is raised)
__device__ __forceinline__ void rl_clamp_list(const long long* cand_off, long long n_cand, int b, long long& lo, long long& len, int* flags) {
    const long long o0 = cand_off[b], o1 = cand_off[b + 1];
    lo = min(max(o0, 0ll), n_cand);
    const long long hi = min(max(o1, 0ll), n_cand);
    len = hi > lo ? hi - lo : 0;
    if (flags != nullptr && (lo != o0 || hi != o1 || hi < lo)) atomicOr(flags, AMID_FLAG_INDEX_RANGE);
}
__device__ __forceinline__ int rl_units(long long len, int per) {
    const long long tiles = (len + RL_TILE - 1) / RL_TILE;
    return (int)((tiles + per - 1) / per);
}

// ONE workgroup: unit_pre[b] = units of the rows before b; unit_pre[B] = all.  A thread sums the unit counts of `chunk` consecutive rows, one
// 256-wide scan joins the threads' sums, the thread walks its rows again.  Offsets that do not rise (clamped or not) can name overlapping
// lists, with more units than the host's bound sized the workspace for: the prefix is cut at that bound (the rows behind the cut lose
// units, the last of them maybe its tail) and the flag is raised.
__device__ __forceinline__ void rl_unit_prefix(const long long* cand_off, long long n_cand, int B, int per, int unit_bound, int* unit_pre,
                                               int* flags) {
    __shared__ long long sc[FR_THREADS];
    const int tid = threadIdx.x;
    const int chunk = (B + FR_THREADS - 1) / FR_THREADS;
    const int b0 = (int)min((long long)B, (long long)tid * chunk), b1 = (int)min((long long)B, (long long)b0 + chunk);
    long long mine = 0;
    for (int b = b0; b < b1; ++b) {
        long long lo, len;
        rl_clamp_list(cand_off, n_cand, b, lo, len, nullptr);
        mine += rl_units(len, per);
    }
    sc[tid] = mine;
    __syncthreads();
    for (int d = 1; d < FR_THREADS; d <<= 1) {                     // inclusive scan
        const long long v = tid >= d ? sc[tid - d] : 0;
        __syncthreads();
        sc[tid] += v;
        __syncthreads();
    }
    long long run = sc[tid] - mine;
    for (int b = b0; b < b1; ++b) {
        long long lo, len;
        rl_clamp_list(cand_off, n_cand, b, lo, len, nullptr);
        unit_pre[b] = (int)min(run, (long long)unit_bound);
        run += rl_units(len, per);
    }
    if (tid == FR_THREADS - 1) {
        unit_pre[B] = (int)min(sc[tid], (long long)unit_bound);
        if (sc[tid] > unit_bound) atomicOr(flags, AMID_FLAG_INDEX_RANGE);
    }
}

// the row of a unit: unit_pre[b] <= unit < unit_pre[b + 1]
__device__ __forceinline__ int rl_row_of_unit(const int* unit_pre, int B, int unit) {
    int b = 0, hi = B - 1;
    while (b < hi) {
        const int mid = (b + hi + 1) >> 1;
        if (unit_pre[mid] <= unit) b = mid; else hi = mid - 1;
    }
    return b;
}

// ---- host side ------------------------------------------------------------------------------------------------------------------------------
// what the host knows about the number of tiles: every row adds at most one partly filled tile
static inline long long rl_tile_bound(int B, long long n_cand) { return (n_cand + RL_TILE - 1) / RL_TILE + B; }
static inline int rl_per_for(int B, long long n_cand, int target_units) {
    return (int)std::max(1ll, (rl_tile_bound(B, n_cand) + target_units - 1) / target_units);
}
// units <= sum over the rows of ceil(tiles / per) <= tile bound / per + B <= target + B, and <= the tile bound; with RL_UNITS for the target
// (which is never above it) neither falls when B or n_cand grows
static inline long long rl_unit_bound(int B, long long n_cand) { return std::min((long long)RL_UNITS + B, rl_tile_bound(B, n_cand)); }
static inline size_t rl_align(size_t x) { return (x + 255) & ~(size_t)255; }

}  // namespace amid
