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
#include "ragged_lists.h"

namespace amid {

#pragma clang fp contract(off)

// (RL_TILE, RL_GRID, RL_UNITS -- the default and maximum of amid_rank_lists_target_workgroups --, the list and the walk over rows, tiles and
// units: ragged_lists.h, which diversify.hip shares)
constexpr int RL_RPL = 4;               // candidates per group of eight lanes and pass: a pass covers 32 RL_RPL = 128 entries of the tile
constexpr int RL_PASS = (FR_THREADS >> 3) * RL_RPL;

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
    rl_clamp_list(a.cand_off, a.n_cand, b, lo, len, raise ? a.flags : nullptr);
}

// ---- per row: offsets, au, padding; the prefix of the unit counts ---------------------------------------------------------------------------------
template <int HID>
__global__ __launch_bounds__(FR_THREADS) void rl_prep_kernel(const RlArgs a) {
    const int tid = threadIdx.x;
    const int n_wg = gridDim.x - 1;                                    // workgroups over the rows; the last one scans
    if ((int)blockIdx.x == n_wg) {                                     // unit_pre[b] = units of the rows before b; unit_pre[B] = all
        rl_unit_prefix(a.cand_off, a.n_cand, a.B, a.per, a.unit_bound, a.unit_pre, a.flags);
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
        const int b = rl_row_of_unit(a.unit_pre, a.B, unit);           // (uniform)
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
            rl_merge_units(c, K, ps, pk, nu);
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
static inline int rl_per(int B, long long n_cand) { return rl_per_for(B, n_cand, rl_target_units); }

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
