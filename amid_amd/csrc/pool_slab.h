// The PREPARED form of an input pool (pool_prepare.hip writes it, adam.hip's prepared step head reads it): per batch of the pool one slab of
// int32 words holding what the step head's packing role and the five phases of the step's index sort leave for their consumers -- all of it a
// function of the batch alone, so it is made once per pool fill instead of once per step.  Sections start on 16-byte borders:
//   hdr [16]            [0] n_uniq, [1] the batch's out-of-range flag (ids outside [0, n_rows) are stored as 0)
//   idx_all [n_idx]     the full index list [seq_d1 B T | seq_d2 B T | items B NI]
//   idx_c, row_c [n_c]  the compact list (every sample's own-domain sequence, then the items) and its rows in the full layout
//   live [B + 1]        amid_live_list_i32
//   pos_sorted [n_c]    row_c in the order of the stable sort of idx_c
//   uniq_ids [n_c], seg_off [n_c + 1], seg_of [n_c]     the runs of the sorted ids (the first n_uniq / n_uniq + 1 entries of the first two)
#pragma once
#include "common.h"

namespace amid {

struct SlabLayout {
    int n_idx, n_c, B;
    int idx_all, idx_c, row_c, live, pos_sorted, uniq_ids, seg_off, seg_of;      // offsets in ints from the slab's base
    int ints;                                                                   // a slab's length, a multiple of 64 ints
};
constexpr int SLAB_HDR_INTS = 16;

__host__ __device__ inline SlabLayout slab_layout(int B, int T, int n_neg) {
    SlabLayout L;
    L.B = B;
    L.n_idx = 2 * B * T + B * (1 + n_neg);
    L.n_c = B * T + B * (1 + n_neg);
    int o = SLAB_HDR_INTS;
    auto take = [&](int n) { const int at = o; o += (n + 3) & ~3; return at; };
    L.idx_all = take(L.n_idx);
    L.idx_c = take(L.n_c);
    L.row_c = take(L.n_c);
    L.live = take(B + 1);
    L.pos_sorted = take(L.n_c);
    L.uniq_ids = take(L.n_c);
    L.seg_off = take(L.n_c + 1);
    L.seg_of = take(L.n_c);
    L.ints = (o + 63) & ~63;
    return L;
}

// ---- a batch of the pool as the kernels read it ----
struct PoolBatch {          // a packed batch image (engine_io.py pack_epoch): [i_node B][neg B n_neg][seq_d1 B T][seq_d2 B T][domain B] ...
    const long long* __restrict__ src;
    int B, T, n_neg;
    long long n_rows;
    __device__ __forceinline__ int n_compact() const { return B * T + B * (1 + n_neg); }
    // compact position p: sample b's own-domain sequence at p = b T + t, then the items.  Returns the id (0 when out of range, as the
    // packing launches do -- they raise the flag) and the row of the full [2 B T + B NI] layout its gradient stands in
    __device__ __forceinline__ int at(int p, int& row) const {
        const int M = B * T, NI = 1 + n_neg, items0 = B + B * n_neg;
        int word;
        if (p < M) {
            const int b = p / T;
            const int dom = src[items0 + 2 * M + b] != 0 ? 1 : 0;
            word = items0 + dom * M + p;
            row = dom * M + p;
        } else {
            const int j = p - M, b = j / NI, k = j - b * NI;
            word = k == 0 ? b : B + b * n_neg + (k - 1);
            row = 2 * M + j;
        }
        const long long v = src[word];
        return (v < 0 || v >= n_rows) ? 0 : (int)v;
    }
};
struct PoolKeys { PoolBatch pb; __device__ __forceinline__ int operator()(int k) const { int row; return pb.at(k, row); } };

}  // namespace amid
