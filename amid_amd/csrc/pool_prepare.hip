// An input pool PREPARED at pool fill (amid_pool_prepare_i32): what the step head's packing role and the five phases of the step's index sort
// compute from a batch -- the index lists, the live list, the stable sort of the compact list with its runs -- depends on the batch alone, not
// on the parameters, the step number or the Adam state, and the pool holds a whole epoch's batches in HBM (engine_io.py set_input_pool).  So it
// is computed for ALL batches of the pool in five launches with the batch index in the grid, into one slab per batch (pool_slab.h), and a train
// step's head copies its batch's slab into the plan's buffers (adam.hip step_head_prepared_kernel) instead of building it: sixty chains of
// dependent loads per epoch become one pass off the step's critical path.  The sort is the two-pass stable radix sort of sort_phases.h itself,
// phase by phase as the step's riders run it (1 024-bin build: keys below 2^20), on a private workspace per batch: the same permutation.
#include "common.h"
#include "sort_phases.h"
#include "live_list.h"
#include "pool_slab.h"

namespace amid {

// per-batch workspace of the sort (ints; zero when a prepare starts -- the entry clears it): state | stot0 x 2 | stot1 | counts0 | counts1 |
// hstatus | keys0 | vals0 | keys1
struct PrepScratch {
    int state, stot0, stot0_copy, stot1, counts0, counts1, hstatus, keys0, vals0, keys1;
    long long ints;
};
static inline PrepScratch prep_scratch(int n_c, int b0, int b1) {
    const int nblk = (n_c + SORT_TILE - 1) / SORT_TILE, nsup = (nblk + OS_SUPER - 1) / OS_SUPER;
    PrepScratch s;
    long long o = 0;
    auto take = [&](long long n) { const long long at = o; o += (n + 3) & ~3LL; return (int)at; };
    s.state = take(OS_STATE_INTS);
    s.stot0_copy = ((nsup << b0) + 3) & ~3;
    s.stot0 = take(2LL * s.stot0_copy);
    s.stot1 = take((long long)nsup << b1);
    s.counts0 = take((long long)nblk << b0);
    s.counts1 = take((long long)nblk << b1);
    s.hstatus = take(nblk);
    s.keys0 = take(n_c); s.vals0 = take(n_c); s.keys1 = take(n_c);
    s.ints = (o + 63) & ~63LL;
    return s;
}
constexpr int PREP_ERR_WORD = 8;          // state[8] of a batch's workspace collects its out-of-range flag (the sort uses state[2 .. 7])

struct PrepArgs {
    const long long* pool; long long stride; int n_pool, in_words;
    int B, T, n_neg; long long n_rows;
    int* slab; long long slab_stride;
    int* scratch; long long scr_stride;
    SlabLayout lay;
    SortPlan plan0;                       // batch 0's plan: batch b's pointers lie b strides further
    int npk;
};

__device__ __forceinline__ SortPlan prep_plan(const PrepArgs& a, int b) {
    SortPlan sp = a.plan0;
    const long long ds = (long long)b * a.slab_stride, dw = (long long)b * a.scr_stride;
    sp.idx += ds; sp.rows += ds; sp.pos_sorted += ds; sp.uniq_ids += ds; sp.seg_off += ds; sp.seg_of += ds; sp.n_uniq += ds;
    sp.state += dw; sp.stot0 += dw; sp.stot1 += dw; sp.counts0 += dw; sp.counts1 += dw; sp.hstatus += dw;
    sp.keys0 += dw; sp.vals0 += dw; sp.keys1 += dw;
    return sp;
}

// PHASE 1: workgroups [0, nblk) count pass 0's digits with the keys read from the batch image (as the step head's riders do), the next npk
// pack the lists.  PHASE 2 .. 5: the sort's later phases; the first workgroup of phase 5 also stores the batch's flag.
template <int PHASE>
__global__ __launch_bounds__(SORT_THREADS) void pool_prepare_kernel(const PrepArgs a) {
    __shared__ __attribute__((aligned(16))) int lds[(sizeof(SortScatterLds<1024>) + 15) / 4];
    const int b = blockIdx.y;
    const SortPlan sp = prep_plan(a, b);
    if constexpr (PHASE == 1) {
        PoolBatch pb;
        pb.src = a.pool + (long long)b * a.stride; pb.B = a.B; pb.T = a.T; pb.n_neg = a.n_neg; pb.n_rows = a.n_rows;
        if ((int)blockIdx.x < sp.nblk) {
            os_count_block<1024>(blockIdx.x, sp.nblk, PoolKeys{pb}, sp.g0, sp.state, sp.counts0, sp.stot0, sp.stot0_copy, sp.n_zero_a, sp.counts1,
                                 sp.n_counts1, sp.stot1, sp.n_stot1, (int*)sp.hstatus, lds);
            return;
        }
        const int pk = blockIdx.x - sp.nblk;
        int* const s = a.slab + (long long)b * a.slab_stride;
        const SlabLayout& L = a.lay;
        const int M = a.B * a.T, NI = 1 + a.n_neg, n_items = a.B * a.n_neg, n_index_words = a.B + n_items + 2 * M;
        if (pk == a.npk - 1) live_list_block(pb.src + n_index_words, a.B, s + L.live);
        bool bad = false;
        for (int i = pk * SORT_THREADS + threadIdx.x; i < n_index_words; i += a.npk * SORT_THREADS) {
            long long v = pb.src[i];
            int dst;
            if (i < a.B) dst = 2 * M + i * NI;
            else if (i < a.B + n_items) { const int j = i - a.B; dst = 2 * M + (j / a.n_neg) * NI + 1 + (j % a.n_neg); }
            else dst = i - a.B - n_items;
            if (v < 0 || v >= a.n_rows) { bad = true; v = 0; }
            s[L.idx_all + dst] = (int)v;
        }
        if (bad) atomicOr(&sp.state[PREP_ERR_WORD], 1);
        for (int p = pk * SORT_THREADS + threadIdx.x; p < L.n_c; p += a.npk * SORT_THREADS) {
            int row;
            s[L.idx_c + p] = pb.at(p, row);
            s[L.row_c + p] = row;
        }
    } else {
        if constexpr (PHASE == 5) {
            if (blockIdx.x == 0 && threadIdx.x == 0) a.slab[(long long)b * a.slab_stride + 1] = sp.state[PREP_ERR_WORD];     // (final: phase 1's launch is over)
        }
        sort_phase_bins<1024, PHASE>(sp, blockIdx.x, lds);
    }
}

}  // namespace amid

using namespace amid;

static int prep_bits(long long n_rows, int& b0, int& b1) {
    int bits = 1;
    while (bits < 31 && (1LL << bits) < n_rows) ++bits;
    if (bits > 20) return AMID_ERR_UNSUPPORTED;           // the 1 024-bin build: keys below 2^20
    if (bits < 2) bits = 2;
    b0 = (bits + 1) / 2; b1 = bits - b0;
    return AMID_OK;
}

// ints of one batch's slab (pool_slab.h); 0 for a bad shape
extern "C" long long amid_pool_slab_ints(int B, int T, int n_neg) {
    if (B <= 0 || T <= 0 || n_neg <= 0 || 2LL * B * T + (long long)B * (1 + n_neg) > (1LL << 28)) return 0;
    return slab_layout(B, T, n_neg).ints;
}

// bytes of the prepare's workspace for a pool of n_pool batches; 0 where amid_pool_prepare_i32 does not cover the shape (keys of 2^20 and more)
extern "C" long long amid_pool_prepare_workspace_bytes(int n_pool, int B, int T, int n_neg, long long n_rows) {
    int b0, b1;
    if (n_pool <= 0 || n_rows <= 0 || amid_pool_slab_ints(B, T, n_neg) == 0 || prep_bits(n_rows, b0, b1) != AMID_OK) return 0;
    return prep_scratch(slab_layout(B, T, n_neg).n_c, b0, b1).ints * 4 * n_pool;
}

// pool [n_pool][pool_stride] (rows = SasrecEngine.pack_batch images of in_words words) -> slabs [n_pool][slab_stride] ints (slab_stride >=
// amid_pool_slab_ints, a multiple of 4; 16-byte aligned base).  workspace: amid_pool_prepare_workspace_bytes, 16-byte aligned; cleared here.
extern "C" int amid_pool_prepare_i32(const long long* pool, long long pool_stride, int n_pool, int in_words, int B, int T, int n_neg,
                                     long long n_rows, int* slab, long long slab_stride, void* workspace, void* stream) {
    AMID_CHECK_ARG(pool && slab && workspace && n_pool > 0 && n_pool <= 65535 && B > 0 && T > 0 && n_neg > 0 && n_rows > 0);
    AMID_CHECK_ARG(amid_pool_slab_ints(B, T, n_neg) > 0 && in_words >= B + B * n_neg + 2 * B * T + B && pool_stride >= in_words);
    const SlabLayout lay = slab_layout(B, T, n_neg);
    AMID_CHECK_ARG(slab_stride >= lay.ints && (slab_stride & 3) == 0 && (((unsigned long long)slab | (unsigned long long)workspace) & 15) == 0);
    int b0, b1;
    if (int e = prep_bits(n_rows, b0, b1)) return e;
    const PrepScratch sc = prep_scratch(lay.n_c, b0, b1);
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(workspace, 0, (size_t)sc.ints * 4 * n_pool, s) != hipSuccess) return AMID_ERR_ARG;
    PrepArgs a;
    a.pool = pool; a.stride = pool_stride; a.n_pool = n_pool; a.in_words = in_words; a.B = B; a.T = T; a.n_neg = n_neg; a.n_rows = n_rows;
    a.slab = slab; a.slab_stride = slab_stride; a.scratch = (int*)workspace; a.scr_stride = sc.ints; a.lay = lay;
    const int nblk = (lay.n_c + SORT_TILE - 1) / SORT_TILE, nsup = (nblk + OS_SUPER - 1) / OS_SUPER;
    int* const w = (int*)workspace;
    SortPlan& sp = a.plan0;
    sp.idx = slab + lay.idx_c; sp.rows = slab + lay.row_c; sp.n = lay.n_c; sp.nblk = nblk; sp.nsup = nsup;
    sp.g0 = OsGeom{lay.n_c, nblk, 0, b0, b0, b1};
    sp.g1 = OsGeom{lay.n_c, nblk, b0, b1, 0, b0};
    sp.state = w + sc.state; sp.stot0 = w + sc.stot0; sp.stot1 = w + sc.stot1; sp.counts0 = w + sc.counts0; sp.counts1 = w + sc.counts1;
    sp.hstatus = (unsigned*)(w + sc.hstatus); sp.keys0 = w + sc.keys0; sp.vals0 = w + sc.vals0; sp.keys1 = w + sc.keys1;
    sp.pos_sorted = slab + lay.pos_sorted; sp.uniq_ids = slab + lay.uniq_ids; sp.seg_off = slab + lay.seg_off; sp.seg_of = slab + lay.seg_of;
    sp.n_uniq = slab;                                              // hdr[0]
    sp.n_counts1 = (long long)nblk << b1; sp.n_stot1 = nsup << b1; sp.n_zero_a = nsup << b0; sp.stot0_copy = sc.stot0_copy;
    int npk = (lay.n_idx + 2047) / 2048;
    if (npk < 2) npk = 2;
    if (npk > 32) npk = 32;
    a.npk = npk;
    pool_prepare_kernel<1><<<dim3(nblk + npk, n_pool), SORT_THREADS, 0, s>>>(a);
    pool_prepare_kernel<2><<<dim3(nblk, n_pool), SORT_THREADS, 0, s>>>(a);
    pool_prepare_kernel<3><<<dim3(nblk, n_pool), SORT_THREADS, 0, s>>>(a);
    pool_prepare_kernel<4><<<dim3(nblk, n_pool), SORT_THREADS, 0, s>>>(a);
    pool_prepare_kernel<5><<<dim3(nblk, n_pool), SORT_THREADS, 0, s>>>(a);
    AMID_LAUNCH_CHECK();
    return AMID_OK;
}
