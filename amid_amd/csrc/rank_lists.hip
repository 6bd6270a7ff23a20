// Ranking each row's OWN candidate list through predictModule: row b's vector against cand[cand_off[b] .. cand_off[b + 1]), ragged lists from
// empty to tens of thousands of entries, duplicates allowed.  p(u, c) = sigmoid(w2 . relu((W1[:, :D] u + b1) + W1[:, D:] E[c]) + b2).
//
// Nothing is shared between rows here (full_rank.hip and audience.hip live on a catalogue every row shares: one half is formed once per
// candidate and a pair costs hid operations).  Every (row, candidate) pair pays its own item half, D x hid fmas on one gathered table row,
// so the work is the gather and those fmas, and the rest is balancing ragged lists without the host reading an offset.  Every piece of the
// arithmetic is head_parts.h's (the user half: user_half_chain joined by group_sum<8>, then + b1[j], as fr_user_kernel forms it; the item
// half: item_half_chain's fmas in item_half_chain's order joined by group_sum<8>, as fr_items_kernel forms it; head_logit_p): a score is
// bit-identical to what amid_topk_f32 and amid_audience_topk_f32 give for the same vector and the same table row.
//
// A list is cut into tiles of RL_TILE entries and a row's tiles into UNITS of `per` consecutive tiles (per = ceil(tile bound / target
// workgroups), from the host's n_cand and B alone).  Launches (all on the caller's stream, no host synchronisation):
//   rl_prep_kernel    persistent workgroups over the rows: the offsets clamped into [0, n_cand]; au[b] = W1[:, :D] u_b + b1 into the
//                     workspace; an empty list's row of the result written as padding (an empty list costs its workgroup one look at two
//                     offsets).  One more workgroup: the exclusive prefix unit_pre [B + 1] of the rows' unit counts
//   rl_score_kernel   persistent workgroups over the units (the row of a unit: binary search in unit_pre).  W1[:, D:]^T staged in LDS once
//                     per workgroup.  A tile goes in two passes of 128 candidates.  Eight lanes a candidate, four candidates a group of
//                     eight: lane `part` loads the 16-byte column quads 4 part + 32 k of its four table rows straight into registers (the
//                     eight lanes of a candidate read 128 contiguous bytes a step, D / 8 such loads in flight a lane) and walks the hid
//                     outputs four at a time -- one 16-byte LDS read of W1^T per sixteen fmas.  group_sum<8> leaves every sum in all eight
//                     lanes: lane `part` < 4 stores the sums of candidate `part` of the four to LDS, and a thread per candidate of the
//                     pass forms the logit.  Then a thread per entry of the tile: list_scores, the history test (binary search of
//                     own(b)), and the offer to the unit's running best-K list
//   rl_merge_kernel   persistent workgroups over the rows: the row's units' lists through the same merge -> ids / scores / positions [B, K]
// The best-K list is topk_list.h's in shape (a list in LDS, newcomers merged by a bitonic sort of list + newcomers, the merges deferred as
// audience.hip's au_offer defers them) with a 64-bit key in place of the int id: (id << 32) | position.  The order -- larger score first,
// ties to the lower id, further ties to the lower position -- is total over a list's entries, so the k best and their order do not depend
// on how the list was cut into tiles and units or on which workgroup took which unit.
#include <algorithm>
#include "head_parts.h"
#include "topk_list.h"
#include "amid_hip.h"

namespace amid {

#pragma clang fp contract(off)

constexpr int RL_TILE = 256;            // candidates per tile: one per thread of the offer
constexpr int RL_RPL = 4;               // candidates per group of eight lanes and pass: a pass covers 32 RL_RPL = 128 entries of the tile
constexpr int RL_PASS = (FR_THREADS >> 3) * RL_RPL;
constexpr int RL_PEND = 256;            // newcomers a list collects between two merges (list + pending <= the 512 of the merge buffer)
constexpr int RL_GRID = 1024;           // persistent workgroups of the score launch at most
constexpr int RL_UNITS = 2048;          // target number of units (default and maximum of amid_rank_lists_target_workgroups)
constexpr unsigned long long RL_KEY_NONE = ~0ull;       // an empty list slot (sorts after every entry)

struct RlArgs {
    const float* u; long long u_dom_stride;     // row b's vector: u + domain(b) * u_dom_stride + b * D
    const long long* domain;                    // [B]
    const long long* cand; const long long* cand_off; long long n_cand;
    const long long* own; const int* own_off; const int* rows;   // own(b) = own[own_off[rows[b]] .. own_off[rows[b] + 1]), or own null
    const float* table; long long n_rows;
    const float* w1; const float* b1; const float* w2; const float* b2;
    int B, D, hid, K;
    int per;                                    // tiles per unit
    int unit_bound;                             // rows of part_s / part_k: the prefix never counts more units than this
    int* flags;
    float* au;                                  // workspace [B][hid]
    int* unit_pre;                              // workspace [B + 1]
    float* part_s; unsigned long long* part_k;  // workspace [units][K]
    float* list_scores;                         // [n_cand] or null
    long long* out_ids; float* out_s; long long* out_pos;        // [B][K] or null (K = 0)
};

// row b's list [lo, lo + len) with both offsets clamped into [0, n_cand]; an offset outside, or a falling pair (an empty list), raises the flag
__device__ __forceinline__ void rl_list_of(const RlArgs& a, int b, long long& lo, long long& len, bool raise) {
    const long long o0 = a.cand_off[b], o1 = a.cand_off[b + 1];
    lo = min(max(o0, 0ll), a.n_cand);
    const long long hi = min(max(o1, 0ll), a.n_cand);
    len = hi > lo ? hi - lo : 0;
    if (raise && (lo != o0 || hi != o1 || hi < lo)) atomicOr(a.flags, AMID_FLAG_INDEX_RANGE);
}
__device__ __forceinline__ int rl_units_of(const RlArgs& a, long long len) {
    const long long tiles = (len + RL_TILE - 1) / RL_TILE;
    return (int)((tiles + a.per - 1) / a.per);
}

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

// ---- per row: offsets, au, padding; the prefix of the unit counts ---------------------------------------------------------------------------------
template <int HID>
__global__ __launch_bounds__(FR_THREADS) void rl_prep_kernel(const RlArgs a) {
    const int tid = threadIdx.x;
    const int n_wg = gridDim.x - 1;                                    // workgroups over the rows; the last one scans
    if ((int)blockIdx.x == n_wg) {                                     // unit_pre[b] = units of the rows before b; unit_pre[B] = all
        // a thread sums the unit counts of `chunk` consecutive rows, one 256-wide scan joins the threads' sums, the thread walks its rows again
        // Offsets that do not rise (clamped or not) can name overlapping lists, with more units than the host's bound sized the workspace
        // for: the prefix is cut at that bound (the rows behind the cut lose units, the last of them maybe its tail) and the flag is raised.
        __shared__ long long sc[FR_THREADS];
        const int chunk = (a.B + FR_THREADS - 1) / FR_THREADS;
        const int b0 = (int)min((long long)a.B, (long long)tid * chunk), b1 = (int)min((long long)a.B, (long long)b0 + chunk);
        long long mine = 0;
        for (int b = b0; b < b1; ++b) {
            long long lo, len;
            rl_list_of(a, b, lo, len, false);
            mine += rl_units_of(a, len);
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
            rl_list_of(a, b, lo, len, false);
            a.unit_pre[b] = (int)min(run, (long long)a.unit_bound);
            run += rl_units_of(a, len);
        }
        if (tid == FR_THREADS - 1) {
            a.unit_pre[a.B] = (int)min(sc[tid], (long long)a.unit_bound);
            if (sc[tid] > a.unit_bound) atomicOr(a.flags, AMID_FLAG_INDEX_RANGE);
        }
        return;
    }
    const int D = a.D, part = tid & 7;
    for (int b = blockIdx.x; b < a.B; b += n_wg) {
        long long lo, len;
        rl_list_of(a, b, lo, len, tid == 0);
        if (len == 0) {                                                // (uniform) no unit will touch this row
            if (a.out_ids != nullptr)
                for (int k = tid; k < a.K; k += FR_THREADS) {
                    const long long o = (long long)b * a.K + k;
                    a.out_ids[o] = -1; a.out_s[o] = -INFINITY; a.out_pos[o] = -1;
                }
            continue;
        }
        const float* ub = a.u + (a.domain[b] != 0 ? 1 : 0) * a.u_dom_stride + (long long)b * D;
        for (int o0 = 0; o0 < HID; o0 += FR_THREADS >> 3) {            // (uniform trip count: the shuffles need every lane)
            const int j = o0 + (tid >> 3);
            const bool on = j < HID;
            float acc = on ? user_half_chain(a.w1 + (long long)j * 2 * D, 1, ub, D, part) : 0.f;
            acc = group_sum<8>(acc);
            if (on && part == 0) a.au[(long long)b * HID + j] = acc + a.b1[j];
        }
    }
}

// ---- the scores of a unit's tiles and its best-K list -----------------------------------------------------------------------------------------------
// W1[:, D:]^T in LDS as w1t [D][HID + 4], element e = 32 k + 4 p + c in row 32 k + 8 c + p: at a step (k, c) the eight lanes p of a candidate
// read eight CONSECUTIVE rows, whose 16-byte reads of one output quad lie on disjoint banks (row stride HID + 4 = 20 / 36 / 68 words: eight
// rows start at eight different multiples of 4 mod 32)
__device__ __forceinline__ int rl_w1t_row(int e) { return (e & ~31) | ((e & 3) << 3) | ((e >> 2) & 7); }

// LDS of the score launch: the list's (rl_list_lds_bytes) | w1t [D][HID + 4] | au [64] | p [RL_TILE] | ids [RL_TILE] (8-byte) |
// ci [RL_PASS][HID + 1]: the item halves of a pass
__host__ __device__ inline size_t rl_score_lds_bytes(int D, int hid, int K) {
    return rl_list_lds_bytes(K) + (size_t)4 * ((size_t)D * (hid + 4) + 64 + RL_TILE + (size_t)RL_PASS * (hid + 1)) + (size_t)8 * RL_TILE;
}

template <int HID, int D>
__global__ __launch_bounds__(FR_THREADS) void rl_score_kernel(const RlArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char sm_raw[];
    constexpr int LDW = HID + 4, NQ = D / 32;
    const int K = a.K, tid = threadIdx.x, part = tid & 7, g = tid >> 3;
    const RlLds c = rl_carve(sm_raw, K);
    float* w1t = c.rest;                                               // (16-byte aligned: rl_carve)
    float* au_s = w1t + D * LDW;
    float* p_s = au_s + 64;
    long long* id_s = reinterpret_cast<long long*>(p_s + RL_TILE);
    float* ci_s = reinterpret_cast<float*>(id_s + RL_TILE);
    const int n_units = a.unit_pre[a.B];
    if ((int)blockIdx.x >= n_units) return;                            // (uniform) few units: nothing to stage W1^T for
    for (int x = tid; x < HID * D; x += FR_THREADS) {
        const int j = x / D, e = x - j * D;
        w1t[rl_w1t_row(e) * LDW + j] = a.w1[(long long)j * 2 * D + D + e];
    }
    const float b2 = a.b2[0];
    for (int unit = blockIdx.x; unit < n_units; unit += gridDim.x) {
        int b = 0, hi = a.B - 1;                                       // the row: unit_pre[b] <= unit < unit_pre[b + 1]  (uniform)
        while (b < hi) {
            const int mid = (b + hi + 1) >> 1;
            if (a.unit_pre[mid] <= unit) b = mid; else hi = mid - 1;
        }
        long long lo, len;
        rl_list_of(a, b, lo, len, false);
        const long long n_tiles = (len + RL_TILE - 1) / RL_TILE;
        const long long t0 = (long long)(unit - a.unit_pre[b]) * a.per, t1 = min(n_tiles, t0 + a.per);
        int own_lo = 0, own_hi = 0;
        if (a.own != nullptr) { const int r = a.rows[b]; own_lo = a.own_off[r]; own_hi = a.own_off[r + 1]; }
        if (K > 0) rl_list_reset(c); else __syncthreads();             // (w1t staged; the previous unit's au_s read)
        if (tid < HID) au_s[tid] = a.au[(long long)b * HID + tid];
        for (long long t = t0; t < t1; ++t) {
            const long long p0 = t * RL_TILE;
            const int nn = (int)min((long long)RL_TILE, len - p0);
            const long long my_id = tid < nn ? a.cand[lo + p0 + tid] : -1;
            const bool valid = my_id >= 0 && my_id < a.n_rows;
            if (tid < nn && !valid) atomicOr(a.flags, AMID_FLAG_INDEX_RANGE);
            __syncthreads();                                           // (the previous tile's p_s and id_s are read; au_s written)
            id_s[tid] = valid ? my_id : -1;
            __syncthreads();
            for (int sub = 0; sub < nn; sub += RL_PASS) {              // (uniform)
                // candidate r of this group of eight lanes: entry sub + 4 g + r of the tile; a bad id or a slot past the tile reads nothing
                float4 x[RL_RPL][NQ];
#pragma unroll
                for (int r = 0; r < RL_RPL; ++r) {
                    const long long id = id_s[sub + 4 * g + r];
                    const float* row = a.table + (id < 0 ? 0 : id) * D + 4 * part;
#pragma unroll
                    for (int k = 0; k < NQ; ++k) x[r][k] = id >= 0 ? ld4(row + 32 * k) : make_float4(0.f, 0.f, 0.f, 0.f);
                }
#pragma unroll 1
                for (int j0 = 0; j0 < HID; j0 += 4) {
                    float acc[RL_RPL][4];
#pragma unroll
                    for (int r = 0; r < RL_RPL; ++r)
#pragma unroll
                        for (int q = 0; q < 4; ++q) acc[r][q] = 0.f;
                    // item_half_chain for the outputs j0 .. j0 + 3 of four rows at once: each chain is its output's own,
                    // acc = fmaf(w[e], row[e], acc) over e = 4 part + 32 k + (0, 1, 2, 3): item_half_chain's fmas in item_half_chain's order
#pragma unroll
                    for (int k = 0; k < NQ; ++k) {
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            const float4 wv = ld4(w1t + (32 * k + 8 * q + part) * LDW + j0);
#pragma unroll
                            for (int r = 0; r < RL_RPL; ++r) {
                                const float xv = q == 0 ? x[r][k].x : q == 1 ? x[r][k].y : q == 2 ? x[r][k].z : x[r][k].w;
                                acc[r][0] = fmaf(wv.x, xv, acc[r][0]); acc[r][1] = fmaf(wv.y, xv, acc[r][1]);
                                acc[r][2] = fmaf(wv.z, xv, acc[r][2]); acc[r][3] = fmaf(wv.w, xv, acc[r][3]);
                            }
                        }
                    }
                    // (every lane of the eight holds every sum: lane part < 4 stores candidate `part`'s -- 32 consecutive ci_s rows a wave,
                    // odd stride: no bank conflict)
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const float s0 = group_sum<8>(acc[0][q]), s1 = group_sum<8>(acc[1][q]);
                        const float s2 = group_sum<8>(acc[2][q]), s3 = group_sum<8>(acc[3][q]);
                        const float mine = (part & 2) ? ((part & 1) ? s3 : s2) : ((part & 1) ? s1 : s0);
                        if (part < RL_RPL) ci_s[(4 * g + part) * (HID + 1) + j0 + q] = mine;
                    }
                }
                __syncthreads();
                if (tid < RL_PASS && sub + tid < nn) {                 // a thread per candidate of the pass
                    const float* cr = ci_s + tid * (HID + 1);
                    p_s[sub + tid] = head_logit_p<HID>([&](int j) { return au_s[j]; }, [&](int j) { return cr[j]; }, a.w2, b2);
                }
                __syncthreads();                                       // (p_s written; ci_s read)
            }
            const bool on = tid < nn;
            const float p = on ? p_s[tid] : 0.f;
            if (on && a.list_scores != nullptr) a.list_scores[lo + p0 + tid] = valid ? p : __builtin_nanf("");
            if (K > 0) {
                bool take = on && valid;
                if (take && own_hi > own_lo) {                         // my_id in own(b): sorted unique ids
                    int l = own_lo, h = own_hi;
                    while (l < h) { const int mid = (l + h) >> 1; if (a.own[mid] < my_id) l = mid + 1; else h = mid; }
                    take = !(l < own_hi && a.own[l] == my_id);
                }
                rl_offer(c, K, take, p, ((unsigned long long)my_id << 32) | (unsigned long long)(p0 + tid));
            }
        }
        if (K > 0) {
            __syncthreads();
            const int pn = *c.P.n;
            if (pn > 0) rl_flush(c, K, pn);                            // (uniform) what is still pending
            const int n = *c.L.n;
            const long long o = (long long)unit * K;
            for (int k = tid; k < K; k += FR_THREADS) {
                a.part_s[o + k] = k < n ? c.L.s[k] : -INFINITY;
                a.part_k[o + k] = k < n ? c.L.key[k] : RL_KEY_NONE;
            }
        }
    }
}

// ---- a row's units' lists -> its row of the result ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(FR_THREADS) void rl_merge_kernel(const RlArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char sm_raw[];
    const int K = a.K, tid = threadIdx.x;
    const RlLds c = rl_carve(sm_raw, K);
    for (int b = blockIdx.x; b < a.B; b += gridDim.x) {
        const int u0 = a.unit_pre[b], nu = a.unit_pre[b + 1] - u0;
        if (nu == 0) {                                                 // (uniform) an empty list, or a row behind the cut of the prefix: padding
            for (int k = tid; k < K; k += FR_THREADS) {
                const long long o = (long long)b * K + k;
                a.out_ids[o] = -1; a.out_s[o] = -INFINITY; a.out_pos[o] = -1;
            }
            continue;
        }
        const float* ps = a.part_s + (long long)u0 * K;
        const unsigned long long* pk = a.part_k + (long long)u0 * K;
        const float* rs = ps;                                          // one unit: its list is the row's
        const unsigned long long* rk = pk;
        if (nu > 1) {
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
            __syncthreads();
            const int pn = *c.P.n;
            if (pn > 0) rl_flush(c, K, pn);                            // (uniform)
            for (int k = *c.L.n + tid; k < K; k += FR_THREADS) { c.L.s[k] = -INFINITY; c.L.key[k] = RL_KEY_NONE; }
            __syncthreads();
            rs = c.L.s; rk = c.L.key;
        }
        for (int k = tid; k < K; k += FR_THREADS) {
            const unsigned long long key = rk[k];
            const bool some = key != RL_KEY_NONE;
            const long long o = (long long)b * K + k;
            a.out_ids[o] = some ? (long long)(key >> 32) : -1;
            a.out_s[o] = some ? rs[k] : -INFINITY;
            a.out_pos[o] = some ? (long long)(key & 0xffffffffull) : -1;
        }
    }
}

#pragma clang fp contract(fast)

// ---- host side ------------------------------------------------------------------------------------------------------------------------------
// the score launch's target unit count: RL_UNITS, or what amid_rank_lists_target_workgroups set (tests: fewer = more tiles a unit)
static int rl_target_units = RL_UNITS;
// what the host knows about the number of tiles: every row adds at most one partly filled tile
static inline long long rl_tile_bound(int B, long long n_cand) { return (n_cand + RL_TILE - 1) / RL_TILE + B; }
static inline int rl_per(int B, long long n_cand) {
    return (int)std::max(1ll, (rl_tile_bound(B, n_cand) + rl_target_units - 1) / rl_target_units);
}
// units <= sum over the rows of ceil(tiles / per) <= tile bound / per + B <= target + B, and <= the tile bound; with RL_UNITS for the target
// (which is never above it) neither falls when B or n_cand grows
static inline long long rl_unit_bound(int B, long long n_cand) { return std::min((long long)RL_UNITS + B, rl_tile_bound(B, n_cand)); }
static inline size_t rl_align(size_t x) { return (x + 255) & ~(size_t)255; }

static inline bool rl_sizes_ok(int B, long long n_cand, int k) { return B >= 1 && n_cand >= 0 && n_cand < 0x7fffffffLL && k >= 0 && k <= 256; }
static inline bool rl_shape_ok(int D, int hid) { return (D == 64 || D == 128) && (hid == 16 || hid == 32 || hid == 64); }

// workspace carve: au [B][hid] | unit_pre [B + 1] | part_s [unit bound][k] | part_k [unit bound][k] (8-byte keys)
static long long rl_workspace(int B, long long n_cand, int hid, int k, size_t* off_pre, size_t* off_ps, size_t* off_pk) {
    size_t o = rl_align((size_t)B * hid * 4);
    if (off_pre) *off_pre = o;
    o += rl_align(((size_t)B + 1) * 4);
    const size_t rows = (size_t)rl_unit_bound(B, n_cand) * k;
    if (off_ps) *off_ps = o;
    o += rl_align(rows * 4);
    if (off_pk) *off_pk = o;
    o += rl_align(rows * 8);
    return (long long)o;
}

template <int HID, int D>
static int rl_launch(const RlArgs& a, hipStream_t st) {
    static unsigned long long done_score = 0, done_merge = 0;
    rl_prep_kernel<HID><<<std::min(a.B, RL_GRID) + 1, FR_THREADS, 0, st>>>(a);
    AMID_LAUNCH_CHECK();
    if (a.n_cand == 0) return AMID_OK;                                 // every list is empty: the padding is written
    if (int rc = lds_attr_once((const void*)rl_score_kernel<HID, D>, 160 * 1024, done_score)) return rc;
    const int grid = (int)std::min(rl_unit_bound(a.B, a.n_cand), (long long)RL_GRID);
    rl_score_kernel<HID, D><<<grid, FR_THREADS, rl_score_lds_bytes(D, HID, a.K), st>>>(a);
    AMID_LAUNCH_CHECK();
    if (a.K == 0) return AMID_OK;
    if (int rc = lds_attr_once((const void*)rl_merge_kernel, 160 * 1024, done_merge)) return rc;
    rl_merge_kernel<<<std::min(a.B, RL_GRID), FR_THREADS, rl_list_lds_bytes(a.K), st>>>(a);
    AMID_LAUNCH_CHECK();
    return AMID_OK;
}

}  // namespace amid

using namespace amid;

extern "C" long long amid_rank_lists_workspace_bytes(int B, long long n_cand, int hid, int k) {
    if (!rl_sizes_ok(B, n_cand, k) || (hid != 16 && hid != 32 && hid != 64)) return -1;
    return rl_workspace(B, n_cand, hid, k, nullptr, nullptr, nullptr);
}

extern "C" int amid_rank_lists_target_workgroups(int wgs) {
    const int before = rl_target_units;
    rl_target_units = wgs >= 1 ? std::min(wgs, RL_UNITS) : RL_UNITS;
    return before;
}

extern "C" int amid_rank_lists_f32(const float* u, long long u_dom_stride, const long long* domain_id, int B, const long long* cand,
                                   const long long* cand_off, long long n_cand, const long long* own_items, const int* own_off,
                                   const int* rows, const float* table, long long n_rows, const float* w1, const float* b1, const float* w2,
                                   const float* b2, int D, int hid, int k, void* workspace, int* flags, float* list_scores, long long* ids,
                                   float* scores, long long* positions, void* stream) {
    AMID_CHECK_ARG(u && domain_id && cand_off && table && w1 && b1 && w2 && b2 && workspace && flags);
    const bool topk = ids != nullptr;
    AMID_CHECK_ARG((scores != nullptr) == topk && (positions != nullptr) == topk);
    AMID_CHECK_ARG(topk || list_scores != nullptr);
    AMID_CHECK_ARG(!topk || (k >= 1 && k <= 256));
    AMID_CHECK_ARG(rl_sizes_ok(B, n_cand, 0) && (cand != nullptr || n_cand == 0) && n_rows >= 1 && n_rows <= 0x7fffffffLL && u_dom_stride >= 0);
    AMID_CHECK_ARG(own_items == nullptr || (own_off && rows));
    if (!rl_shape_ok(D, hid)) return AMID_ERR_UNSUPPORTED;
    RlArgs a{};
    a.u = u; a.u_dom_stride = u_dom_stride; a.domain = domain_id; a.B = B;
    a.cand = cand; a.cand_off = cand_off; a.n_cand = n_cand;
    a.own = topk ? own_items : nullptr; a.own_off = own_off; a.rows = rows;
    a.table = table; a.n_rows = n_rows; a.w1 = w1; a.b1 = b1; a.w2 = w2; a.b2 = b2;
    a.D = D; a.hid = hid; a.K = topk ? k : 0; a.per = rl_per(B, n_cand); a.flags = flags;
    a.unit_bound = (int)std::min(rl_unit_bound(B, n_cand), 0x7fffffffLL);
    a.list_scores = list_scores; a.out_ids = ids; a.out_s = scores; a.out_pos = positions;
    size_t o_pre = 0, o_ps = 0, o_pk = 0;
    rl_workspace(B, n_cand, hid, a.K, &o_pre, &o_ps, &o_pk);
    char* ws = (char*)workspace;
    a.au = (float*)ws; a.unit_pre = (int*)(ws + o_pre); a.part_s = (float*)(ws + o_ps); a.part_k = (unsigned long long*)(ws + o_pk);
    const hipStream_t st = (hipStream_t)stream;
    if (D == 64) return hid == 16 ? rl_launch<16, 64>(a, st) : hid == 32 ? rl_launch<32, 64>(a, st) : rl_launch<64, 64>(a, st);
    return hid == 16 ? rl_launch<16, 128>(a, st) : hid == 32 ? rl_launch<32, 128>(a, st) : rl_launch<64, 128>(a, st);
}
