// History sets from the sequences, on the device, with fixed shapes: own(b) = the sorted unique ids of row b's own-domain sequence
// (domain_id[b] != 0 ? seq_d2[b] : seq_d1[b], the pad id kept) as the CSR list amid_topk_f32 / amid_topk_users_f32 read with rows = 0 .. B - 1
// -- the set SASRec.recommend() builds with torch.sort, a boolean-mask gather and a cumsum (a data-dependent shape: one host
// synchronisation a call, and no graph capture).
//
// Two launches on the caller's stream, a workgroup per row in both, no host read, no allocation, no workgroup waits for another:
//   own_count_kernel   the row's ids through a bitonic sort in LDS (padded to a power of two with the largest int64, which sorts behind --
//                      or among -- every real id: the first T entries are the row), adjacent-difference flags, their sum -> cnt[b]
//   own_write_kernel   the same sort and flags again (T <= 2048 ids in LDS: cheaper than a round trip of the sorted rows through HBM), the
//                      row's offset = cnt[0] + .. + cnt[b - 1] (integer sums: any order), the flagged ids at own[offset + rank among the
//                      flags]; own_off[b] = offset, and the last row's workgroup writes own_off[B]
// Words of own past own_off[B] are not written.
#include <climits>
#include "common.h"

namespace amid {

constexpr int OWN_THREADS = 256;
constexpr int OWN_MAX_T = 2048;          // ids of one row in LDS (16 KB) and at most 8 per thread

// s[0 .. P): the row's T ids, sorted ascending (signed), behind them P - T copies of LLONG_MAX.  P: the power of two >= T, >= 2.
__device__ __forceinline__ void own_sort_row(const long long* __restrict__ row, int T, int P, long long* s) {
    const int tid = threadIdx.x;
    for (int i = tid; i < P; i += OWN_THREADS) s[i] = i < T ? row[i] : LLONG_MAX;
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < (P >> 1); t += OWN_THREADS) {
                const int i = 2 * j * (t / j) + (t % j), l = i + j;
                const long long a = s[i], b = s[l];
                const bool up = (i & k) == 0;                  // this run ends up ascending
                if (up ? b < a : a < b) { s[i] = b; s[l] = a; }
            }
            __syncthreads();
        }
    }
}

// The thread's share of the flags: entries [tid * per, tid * per + per) of the sorted row, per = P / OWN_THREADS rounded up.  Returns the
// number of flagged entries (first occurrences) among them.
__device__ __forceinline__ int own_flags(const long long* s, int T, int per, unsigned& mask) {
    const int i0 = threadIdx.x * per;
    int n = 0;
    mask = 0;
    for (int e = 0; e < per; ++e) {
        const int i = i0 + e;
        if (i < T && (i == 0 || s[i] != s[i - 1])) { mask |= 1u << e; ++n; }
    }
    return n;
}

// Inclusive sum over the workgroup's threads (sc: OWN_THREADS ints of LDS); every thread calls it.  Returns this thread's inclusive sum;
// total = the workgroup's.
__device__ __forceinline__ int own_block_scan(int v, int* sc, int& total) {
    const int tid = threadIdx.x;
    sc[tid] = v;
    __syncthreads();
    for (int d = 1; d < OWN_THREADS; d <<= 1) {
        const int add = tid >= d ? sc[tid - d] : 0;
        __syncthreads();
        sc[tid] += add;
        __syncthreads();
    }
    const int inc = sc[tid];
    total = sc[OWN_THREADS - 1];
    __syncthreads();                                           // (sc may be written again)
    return inc;
}

struct OwnArgs {
    const long long* seq[2];        // [B][T] each
    const long long* domain;        // [B]
    int B, T, P;
    int* cnt;                       // [B]
    long long* own;                 // capacity B * T
    int* own_off;                   // [B + 1]
};

__device__ __forceinline__ const long long* own_row(const OwnArgs& a, int b) {
    return a.seq[a.domain[b] != 0 ? 1 : 0] + (long long)b * a.T;
}

__global__ __launch_bounds__(OWN_THREADS) void own_count_kernel(const OwnArgs a) {
    extern __shared__ __attribute__((aligned(16))) long long own_sm[];
    __shared__ int sc[OWN_THREADS];
    const int b = blockIdx.x;
    own_sort_row(own_row(a, b), a.T, a.P, own_sm);
    unsigned mask;
    int total;
    own_block_scan(own_flags(own_sm, a.T, (a.P + OWN_THREADS - 1) / OWN_THREADS, mask), sc, total);
    if (threadIdx.x == 0) a.cnt[b] = total;
}

__global__ __launch_bounds__(OWN_THREADS) void own_write_kernel(const OwnArgs a) {
    extern __shared__ __attribute__((aligned(16))) long long own_sm[];
    __shared__ int sc[OWN_THREADS];
    const int b = blockIdx.x, tid = threadIdx.x;
    int before = 0;
    for (int r = tid; r < b; r += OWN_THREADS) before += a.cnt[r];
    int off;
    own_block_scan(before, sc, off);                           // the rows in front of this one
    own_sort_row(own_row(a, b), a.T, a.P, own_sm);
    const int per = (a.P + OWN_THREADS - 1) / OWN_THREADS;
    unsigned mask;
    int total;
    const int n = own_flags(own_sm, a.T, per, mask);
    int at = off + own_block_scan(n, sc, total) - n;           // exclusive: where this thread's first flagged id goes
    for (int e = 0; e < per; ++e)
        if (mask & (1u << e)) a.own[at++] = own_sm[tid * per + e];
    if (tid == 0) {
        a.own_off[b] = off;
        if (b == a.B - 1) a.own_off[a.B] = off + total;
    }
}

}  // namespace amid

using namespace amid;

extern "C" int amid_own_from_seq_i64(const long long* seq_d1, const long long* seq_d2, const long long* domain_id, int B, int T, int* cnt,
                                     long long* own, int* own_off, void* stream) {
    AMID_CHECK_ARG(seq_d1 && seq_d2 && domain_id && cnt && own && own_off);
    AMID_CHECK_ARG(B >= 1 && T >= 1 && (long long)B * T <= 0x7fffffffLL);
    if (T > OWN_MAX_T) return AMID_ERR_UNSUPPORTED;
    OwnArgs a;
    a.seq[0] = seq_d1; a.seq[1] = seq_d2; a.domain = domain_id;
    a.B = B; a.T = T; a.cnt = cnt; a.own = own; a.own_off = own_off;
    a.P = 2;
    while (a.P < T) a.P <<= 1;
    const hipStream_t st = (hipStream_t)stream;
    const size_t lds = (size_t)a.P * sizeof(long long);
    own_count_kernel<<<B, OWN_THREADS, lds, st>>>(a);
    AMID_LAUNCH_CHECK();
    own_write_kernel<<<B, OWN_THREADS, lds, st>>>(a);
    AMID_LAUNCH_CHECK();
    return AMID_OK;
}
