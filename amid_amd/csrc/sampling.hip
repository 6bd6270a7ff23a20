// Negative sampling on the device (next-3 of SURVEY.md 8(f); reference: dataset_seq.py:188 / :206 and :198 / :215 --
// `random.sample(item_pool_d - set(own sequence), k)` per sample inside __getitem__, the 2.5 k samples/s host bottleneck).
// One wave per row: each round every lane draws one candidate uniformly from the row's domain pool (Philox, keyed by seed,
// epoch and row), rejects it if it is in the row's own sequence, already accepted, or drawn by a lower lane in this round,
// and the survivors are appended in lane order until k are accepted: uniform without replacement over pool \ own.
// The popularity-weighted form (amid_sample_negatives_weighted_i64) is the same loop over another draw: the
// candidate is pool[j], j the first index whose inclusive weight prefix exceeds t = (r64 x total) >> 64, integers throughout.
#include "common.h"
#include "rng.h"

namespace amid {

constexpr unsigned SITE_NEG = 0x4E45;      // RNG site of the sampler (no dropout site uses it)
constexpr unsigned SITE_NEG_W = 0x4E57;    // RNG site of the popularity-weighted sampler: its own stream, SITE_NEG's stays what it was

struct NegArgs {
    const long long* pool[2]; int n_pool[2];   // sorted unique item ids of each domain (dataset_seq.py:141-142)
    const long long* own;                      // concatenated own-sequence item ids of every row
    const int* own_off;                        // [N + 1]
    const long long* domain;                   // [N]
    long long* out;                            // [N, k]
    int N, k;
    unsigned long long seed; unsigned epoch;
};

// The draw of one lane in one round: which Philox site it reads and how the call's 128 bits pick a pool index.
struct UniformDraw {
    static constexpr unsigned SITE = SITE_NEG;
    // Lemire's multiply-shift maps 32 random bits onto [0, n) (bias < n / 2^32, far below sampling noise)
    __device__ __forceinline__ unsigned index(int, unsigned n, const uint4& rn) const { return (unsigned)(((unsigned long long)rn.x * n) >> 32); }
};

// Popularity-weighted draw.  Host side (dataset_seq.popularity_weights): w = floor(count^power * 65536) + 1 per pool entry (the + 1
// keeps a never-seen id drawable; power 0 is uniform), cum = inclusive prefix sum of w, total = cum[n - 1] < 2^62.  Device side, all
// integers: r64 = (x << 32) | y of the call, t = (r64 * total) >> 64 (the high half of the 64 x 64 product, so 0 <= t < total), and
// the index is the first j with cum[j] > t -- np.searchsorted(cum, t, side="right").  P(j) = w[j] / total up to 2^-64 x total.
// The search is ~log2(n) dependent 8-byte loads per lane out of a prefix of n x 8 bytes that stays in L2 (82 KB for a 10 k pool).
struct WeightedDraw {
    static constexpr unsigned SITE = SITE_NEG_W;
    const long long* cum[2];                   // inclusive prefix sums of the weights, aligned with pool[d]
    unsigned long long total[2];               // cum[d][n_pool[d] - 1]
    __device__ __forceinline__ unsigned index(int dom, unsigned n, const uint4& rn) const {
        const unsigned long long t = __umul64hi(((unsigned long long)rn.x << 32) | rn.y, total[dom]);
        const long long* c = cum[dom];
        unsigned lo = 0, hi = n - 1;           // (hi = n - 1, not n: the answer is never past the last entry, whatever `total` the caller gave)
        while (lo < hi) {
            const unsigned mid = (lo + hi) >> 1;
            if ((unsigned long long)c[mid] > t) hi = mid; else lo = mid + 1;
        }
        return lo;
    }
};

// One wave per row, 4 rows per block.  Each round every lane draws one candidate (Draw), rejects it if it is in the row's own
// sequence, already accepted, or drawn by a lower lane in this round; the survivors are appended in lane order until k are accepted.
// Rejecting repeats of a weighted stream is successive sampling without replacement: every pick is proportional to its weight
// among what is left.
template <class Draw>
__device__ __forceinline__ void sample_rows(const NegArgs& a, const Draw& draw, long long* acc_all) {
    const int wv = threadIdx.x >> 6, lane = lane_id();
    const int r = blockIdx.x * 4 + wv;
    if (r >= a.N) return;
    long long* acc = acc_all + (size_t)wv * a.k;
    const int dom = a.domain[r] != 0;
    const long long* pool = a.pool[dom];
    const unsigned n = (unsigned)a.n_pool[dom];
    const long long* own = a.own + a.own_off[r];
    const int n_own = a.own_off[r + 1] - a.own_off[r];
    int have = 0;
    for (unsigned round = 0; have < a.k && round < 4096u; ++round) {
        const uint4 rn = rng_call(a.seed, ((unsigned long long)r << 20) | ((unsigned long long)round << 6) | lane, Draw::SITE, a.epoch);
        const long long cand = pool[draw.index(dom, n, rn)];
        bool ok = true;
        for (int i = 0; i < n_own && ok; ++i) ok = own[i] != cand;
        for (int i = 0; i < have && ok; ++i) ok = acc[i] != cand;
        // duplicates inside the round: a lane loses to any lower lane holding the same candidate
        for (int l = 0; l < 64; ++l) {
            const long long other = __shfl(cand, l, 64);
            if (l < lane && other == cand) ok = false;
        }
        const unsigned long long m = __ballot(ok);
        const int slot = have + __popcll(m & ((1ull << lane) - 1ull));
        if (ok && slot < a.k) { acc[slot] = cand; a.out[(long long)r * a.k + slot] = cand; }
        have = min(a.k, have + __popcll(m));
    }
    // pool exhausted after 4096 rounds: slot 0 says so.  The uniform path never looks for it: DeviceBatches' constructor refuses any
    // row with k + |own| > |pool| (k <= 2048 eligible ids are all met long before 4096 x 64 uniform draws).  A skewed weighted stream
    // can fall short with enough ids eligible, so DeviceBatches reads column 0 after a popularity draw; a direct caller of either C
    // entry point checks out[r][0] itself
    if (have < a.k && lane == 0) a.out[(long long)r * a.k] = -1;
}

__global__ __launch_bounds__(256) void sample_negatives_kernel(const NegArgs a) {
    extern __shared__ long long acc_all[];                     // [4][k] accepted ids of the 4 rows of this block
    sample_rows(a, UniformDraw{}, acc_all);
}

__global__ __launch_bounds__(256) void sample_negatives_weighted_kernel(const NegArgs a, const WeightedDraw w) {
    extern __shared__ long long acc_all[];
    sample_rows(a, w, acc_all);
}

}  // namespace amid

using namespace amid;

static NegArgs neg_args(const long long* pool_d1, int n_pool_d1, const long long* pool_d2, int n_pool_d2, const long long* own_items,
                        const int* own_off, const long long* domain_id, int N, int k, unsigned long long seed, unsigned epoch, long long* out) {
    NegArgs a;
    a.pool[0] = pool_d1; a.pool[1] = pool_d2; a.n_pool[0] = n_pool_d1; a.n_pool[1] = n_pool_d2;
    a.own = own_items; a.own_off = own_off; a.domain = domain_id; a.out = out; a.N = N; a.k = k; a.seed = seed; a.epoch = epoch;
    return a;
}

extern "C" int amid_sample_negatives_i64(const long long* pool_d1, int n_pool_d1, const long long* pool_d2, int n_pool_d2,
                                         const long long* own_items, const int* own_off, const long long* domain_id, int N, int k,
                                         unsigned long long seed, unsigned epoch, long long* out, void* stream) {
    AMID_CHECK_ARG(pool_d1 && pool_d2 && own_items && own_off && domain_id && out && N > 0 && k > 0 && n_pool_d1 > 0 && n_pool_d2 > 0);
    const size_t lds = (size_t)4 * k * sizeof(long long);
    if (lds > 64 * 1024) return AMID_ERR_UNSUPPORTED;
    const NegArgs a = neg_args(pool_d1, n_pool_d1, pool_d2, n_pool_d2, own_items, own_off, domain_id, N, k, seed, epoch, out);
    sample_negatives_kernel<<<(N + 3) / 4, 256, lds, (hipStream_t)stream>>>(a);
    AMID_LAUNCH_CHECK();
    return AMID_OK;
}

extern "C" int amid_sample_negatives_weighted_i64(const long long* pool_d1, const long long* cum_d1, int n_pool_d1,
                                                  const long long* pool_d2, const long long* cum_d2, int n_pool_d2,
                                                  long long total_d1, long long total_d2,
                                                  const long long* own_items, const int* own_off, const long long* domain_id,
                                                  int N, int k, unsigned long long seed, unsigned epoch, long long* out, void* stream) {
    constexpr long long TOTAL_END = 1ll << 62;
    AMID_CHECK_ARG(pool_d1 && cum_d1 && pool_d2 && cum_d2 && own_items && own_off && domain_id && out && N > 0 && k > 0 && n_pool_d1 > 0 &&
                   n_pool_d2 > 0 && total_d1 > 0 && total_d1 < TOTAL_END && total_d2 > 0 && total_d2 < TOTAL_END);
    const size_t lds = (size_t)4 * k * sizeof(long long);
    if (lds > 64 * 1024) return AMID_ERR_UNSUPPORTED;
    const NegArgs a = neg_args(pool_d1, n_pool_d1, pool_d2, n_pool_d2, own_items, own_off, domain_id, N, k, seed, epoch, out);
    WeightedDraw w;
    w.cum[0] = cum_d1; w.cum[1] = cum_d2; w.total[0] = (unsigned long long)total_d1; w.total[1] = (unsigned long long)total_d2;
    sample_negatives_weighted_kernel<<<(N + 3) / 4, 256, lds, (hipStream_t)stream>>>(a, w);
    AMID_LAUNCH_CHECK();
    return AMID_OK;
}
