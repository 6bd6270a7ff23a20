// The running best-K list of the top-K kernels (full_rank.hip: users against their pools through predictModule; neighbors.hip: exact nearest
// neighbours of fp32 vectors; audience.hip: stored user vectors against an item): a list per query in LDS, and the merge of a tile's newcomers into it by a bitonic sort of (list + newcomers).
// Order: larger score first, ties to the lower id.  Every workgroup that uses it has FR_THREADS threads.
#pragma once
#include "common.h"

namespace amid {

constexpr int FR_THREADS = 256;
constexpr int FR_ID_NONE = 0x7fffffff;  // an empty list slot (sorts after every candidate)

// (s1, i1) ranks before (s2, i2): larger score, ties to the lower id
__device__ __forceinline__ bool fr_before(float s1, int i1, float s2, int i2) { return s1 > s2 || (s1 == s2 && i1 < i2); }

struct FrList { float* s; int* id; int* n; };          // one running best-K list in LDS
struct FrScratch { float* s; int* id; int* wcnt; };    // merge buffer [512] scores, [512] ids; per-wave counts [4]

// The merge step: the list's n entries go to the front of the merge buffer, whose entries [n, total) the caller has written (newcomers; no
// barrier needed in between), the rest up to the next power of two is padded with empty slots, the buffer is sorted best first (bitonic, at
// most 512 entries) and the first min(K, total) entries become the list.  Every thread of the workgroup calls this; it ends in a barrier.
__device__ __forceinline__ void fr_sort_keep(const FrList& L, const FrScratch& S, int K, int n, int total) {
    const int tid = threadIdx.x;
    int size = 2;
    while (size < total) size <<= 1;
    for (int i = tid; i < size; i += FR_THREADS) {
        if (i < n) { S.s[i] = L.s[i]; S.id[i] = L.id[i]; }
        else if (i >= total) { S.s[i] = -INFINITY; S.id[i] = FR_ID_NONE; }
    }
    __syncthreads();
    for (int k = 2; k <= size; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < (size >> 1); t += FR_THREADS) {
                const int i = 2 * j * (t / j) + (t % j), l = i + j;
                const float sa = S.s[i], sb = S.s[l];
                const int ia = S.id[i], ib = S.id[l];
                const bool first = (i & k) == 0;               // this run ends up best-first
                if (first ? fr_before(sb, ib, sa, ia) : fr_before(sa, ia, sb, ib)) {
                    S.s[i] = sb; S.s[l] = sa; S.id[i] = ib; S.id[l] = ia;
                }
            }
            __syncthreads();
        }
    }
    const int keep = min(K, total);
    for (int i = tid; i < keep; i += FR_THREADS) { L.s[i] = S.s[i]; L.id[i] = S.id[i]; }
    if (tid == 0) *L.n = keep;
    __syncthreads();
}

// Offer one candidate per thread (cand: it takes part) to the list; every thread of the workgroup calls this.  Newcomers that beat the
// list's K-th entry (or join a list not yet full) go behind the list in the merge buffer, list + newcomers are sorted (fr_sort_keep) and
// the first K stay.
__device__ __forceinline__ void fr_offer(const FrList& L, const FrScratch& S, int K, bool cand, float s, int id) {
    const int tid = threadIdx.x, lane = lane_id(), w = tid >> 6;
    const int n = *L.n;
    bool beat = cand;
    if (cand && n == K) beat = fr_before(s, id, L.s[K - 1], L.id[K - 1]);
    const unsigned long long m = __ballot(beat);
    if (lane == 0) S.wcnt[w] = __popcll(m);
    __syncthreads();
    int off = 0, tot = 0;
    for (int v = 0; v < FR_THREADS / 64; ++v) { off += v < w ? S.wcnt[v] : 0; tot += S.wcnt[v]; }
    __syncthreads();                                           // (every wave has read the counts before the next call writes them)
    if (tot == 0) return;                                      // (uniform)
    if (beat) {
        const int slot = n + off + __popcll(m & ((1ull << lane) - 1ull));
        S.s[slot] = s; S.id[slot] = id;
    }
    fr_sort_keep(L, S, K, n, n + tot);
}

// LDS of fr_merge_ranges: list [K] scores | [K] ids | n [4] | merge [512] scores | [512] ids | wcnt [4]
__host__ __device__ inline size_t fr_merge_lds_bytes(int K) { return (size_t)4 * (2 * K + 4 + 2 * 512 + 4); }

// The last launch of a top-K: a workgroup merges the n_ranges per-range lists part_s / part_i [n_ranges][B][K] of query b (empty slots:
// FR_ID_NONE) into ids / scores [B][K]; fewer than K entries: id -1, score -inf.  sm: fr_merge_lds_bytes(K) bytes of LDS.
__device__ __forceinline__ void fr_merge_ranges(float* sm, int K, int n_ranges, int B, int b, const float* __restrict__ part_s,
                                                const int* __restrict__ part_i, long long* __restrict__ out_ids, float* __restrict__ out_s) {
    const int tid = threadIdx.x;
    float* ls = sm;
    int* li = reinterpret_cast<int*>(ls + K);
    int* ln = li + K;
    FrScratch S;
    S.s = reinterpret_cast<float*>(ln + 4);
    S.id = reinterpret_cast<int*>(S.s + 512);
    S.wcnt = S.id + 512;
    if (tid == 0) *ln = 0;
    __syncthreads();
    const FrList L{ls, li, ln};
    const long long E = (long long)n_ranges * K;
    for (long long e0 = 0; e0 < E; e0 += FR_THREADS) {
        const long long e = e0 + tid;
        float s = -INFINITY;
        int id = FR_ID_NONE;
        if (e < E) {
            const long long r = e / K, k = e - r * K;
            const long long o = (r * B + b) * K + k;
            s = part_s[o]; id = part_i[o];
        }
        fr_offer(L, S, K, id != FR_ID_NONE, s, id);
    }
    const int n = *ln;
    for (int k = tid; k < K; k += FR_THREADS) {
        out_ids[(long long)b * K + k] = k < n ? (long long)li[k] : -1;
        out_s[(long long)b * K + k] = k < n ? ls[k] : -INFINITY;
    }
}

}  // namespace amid
