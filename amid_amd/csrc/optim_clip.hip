// Gradient clipping for the optimizer of the reference's own loop (amid_amd/optim.py): torch.nn.utils.clip_grad_norm_ over EVERY parameter,
// the item table included, without ever forming the table's dense gradient.
//   amid_grad_sqnorm_f32          sum of g^2 over the flat dense gradient and the step's segment-reduced unique rows [0, *n_uniq)
//   amid_optimizer_step_clip_f32  amid_optimizer_step_f32 (adam.hip) whose gradients are scaled by grad_scale * c,
//                                 c = min(1, max_norm / (sqrt(*sqnorm) + 1e-6)): torch's clip coefficient, read on the device
// The norm is two small launches, not one with a last-block finish: 1.7 MB + a few thousand 512-byte rows is latency-bound either way, the
// finish of a one-launch form needs a ticket that somebody has to zero (a workspace with state), and the second launch is 256 doubles.  The
// sum is taken in double in a fixed order -- thread-sequential, wave shuffles, LDS across waves, then one block over the partials -- with a
// grid that does not depend on the data: no float atomics, the same bits on every run.
#include "common.h"
#include "rng.h"
#include "adam_replay.h"

namespace amid {

constexpr int SQN_BLOCKS = 256;          // partial sums (doubles) in the workspace

__device__ __forceinline__ double sq4(float4 a) {
    return ((double)a.x * a.x + (double)a.y * a.y) + ((double)a.z * a.z + (double)a.w * a.w);
}

// the 256 threads' values added up in a fixed order; the total in thread 0
__device__ __forceinline__ double block_sum_fixed(double x, double* red) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = x;
    __syncthreads();
    double s = 0.0;
    if (threadIdx.x == 0) s = (red[0] + red[1]) + (red[2] + red[3]);
    return s;
}

__global__ __launch_bounds__(256) void grad_sqnorm_partials_kernel(const float* __restrict__ g, long long n, const float* __restrict__ rows,
                                                                   const int* __restrict__ n_uniq_p, int cap, int D, double* __restrict__ part) {
    __shared__ double red[4];
    double acc = 0.0;
    const long long stride = (long long)gridDim.x * blockDim.x * 4;
    const long long i0 = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    for (long long i = i0; i < n; i += stride) {
        if (i + 4 <= n) acc += sq4(ld4(g + i));
        else for (long long k = i; k < n; ++k) acc += (double)g[k] * g[k];
    }
    int U = *n_uniq_p;                                   // rows at or beyond it are never read
    U = U < 0 ? 0 : (U > cap ? cap : U);
    const long long nr = (long long)U * D;               // (D % 4 == 0: whole quads)
    for (long long i = i0; i < nr; i += stride) acc += sq4(ld4(rows + i));
    const double s = block_sum_fixed(acc, red);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
}

__global__ __launch_bounds__(256) void grad_sqnorm_finish_kernel(const double* __restrict__ part, int n_part, float* __restrict__ out) {
    __shared__ double red[4];
    const double x = (int)threadIdx.x < n_part ? part[threadIdx.x] : 0.0;
    const double s = block_sum_fixed(x, red);
    if (threadIdx.x == 0) out[0] = (float)s;
}

// torch.nn.utils.clip_grad_norm_: clip_coef = max_norm / (total_norm + 1e-6), clamped to 1 (float32 tensor arithmetic)
__device__ __forceinline__ float clip_coef(const float* __restrict__ sqnorm, float max_norm) {
    const float c = __fdiv_rn(max_norm, __fadd_rn(__fsqrt_rn(*sqnorm), 1e-6f));
    return c < 1.0f ? c : 1.0f;                          // (max_norm = +inf: exactly 1)
}

// optimizer_step_kernel of adam.hip (the same device functions, the same roles) with the clip coefficient folded into the gradient scale
__global__ __launch_bounds__(256) void optimizer_step_clip_kernel(float* __restrict__ p, float* __restrict__ m, float* __restrict__ v,
                                                                  const float* __restrict__ g, long long n, int dense_blocks,
                                                                  float* __restrict__ table, float* __restrict__ m_tab, float* __restrict__ v_tab,
                                                                  int* __restrict__ last, const int* __restrict__ uniq_ids,
                                                                  const int* __restrict__ n_uniq_p, const float* __restrict__ uniq_grad, int D,
                                                                  const StepState* __restrict__ stp, float grad_scale,
                                                                  const float* __restrict__ sqnorm, float max_norm) {
    __shared__ IdleCoef tab[COEF_TAB];
    const StepState st = *stp;
    const float gs = grad_scale * clip_coef(sqnorm, max_norm);
    if ((int)blockIdx.x < dense_blocks) {
        const AdamCoef c = adam_coef_now(st);
        const long long stride = (long long)dense_blocks * blockDim.x * 4;
        for (long long i = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * 4; i < n; i += stride) {
            if (i + 4 <= n) {
                float4 pp = ld4(p + i), mm = ld4(m + i), vv = ld4(v + i);
                adam_quad(pp, mm, vv, f4scale(ld4(g + i), gs), c);
                st4(p + i, pp); st4(m + i, mm); st4(v + i, vv);
            } else {
                for (long long k = i; k < n; ++k) adam_elem(p[k], m[k], v[k], g[k] * gs, c);
            }
        }
        return;
    }
    const long long t = st.step;
    const int U = *n_uniq_p;
    const int rb = blockIdx.x - dense_blocks, n_rb = gridDim.x - dense_blocks;
    if (rb * 8 >= U) return;
    fill_coef_table(tab, st);
    const AdamCoef cnow = adam_coef_now(st);
    const int sub = threadIdx.x & 31;
    const int q = D >> 2;
    for (int u = rb * 8 + (threadIdx.x >> 5); u < U; u += n_rb * 8) {
        const long long r = uniq_ids[u];
        const long long l = last[r];
        const bool lag = (l > 0 && l < t - 1);
        for (int c = sub; c < q; c += 32) {
            const long long off = r * D + 4 * c;
            float4 pp = ld4(table + off), mm = ld4(m_tab + off), vv = ld4(v_tab + off);
            if (lag) replay_quad(pp, mm, vv, l + 1, t - 1, st, tab);
            adam_quad(pp, mm, vv, f4scale(ld4(uniq_grad + (long long)u * D + 4 * c), gs), cnow);
            st4(table + off, pp); st4(m_tab + off, mm); st4(v_tab + off, vv);
        }
        __builtin_amdgcn_wave_barrier();
        if (sub == 0) last[r] = (int)t;
    }
}

}  // namespace amid

using namespace amid;

extern "C" long long amid_grad_sqnorm_workspace_bytes(void) { return (long long)SQN_BLOCKS * (long long)sizeof(double); }

extern "C" int amid_grad_sqnorm_f32(const float* g_dense, long long n_dense, const float* uniq_grad, const int* n_uniq, int cap, int D,
                                    void* ws, float* out, void* stream) {
    AMID_CHECK_ARG(n_dense >= 0 && (g_dense || n_dense == 0) && uniq_grad && n_uniq && cap >= 0 && D > 0 && (D % 4) == 0 && ws && out);
    // quads are read as one load: both lists start on a 16-byte boundary (the partials are doubles)
    AMID_CHECK_ARG(((uintptr_t)g_dense % 16) == 0 && ((uintptr_t)uniq_grad % 16) == 0 && ((uintptr_t)ws % 8) == 0);
    long long work = (n_dense + (long long)cap * D + 3) / 4;
    long long blocks = (work + 255) / 256;
    if (blocks < 1) blocks = 1;
    if (blocks > SQN_BLOCKS) blocks = SQN_BLOCKS;      // (a function of the sizes alone: the order of the additions is fixed)
    grad_sqnorm_partials_kernel<<<(int)blocks, 256, 0, (hipStream_t)stream>>>(g_dense, n_dense, uniq_grad, n_uniq, cap, D, (double*)ws);
    AMID_LAUNCH_CHECK();
    grad_sqnorm_finish_kernel<<<1, 256, 0, (hipStream_t)stream>>>((const double*)ws, (int)blocks, out);
    AMID_LAUNCH_CHECK();
    return AMID_OK;
}

extern "C" int amid_optimizer_step_clip_f32(float* p, float* m, float* v, const float* g, long long n, float* table, float* m_tab, float* v_tab,
                                            int* last, const int* uniq_ids, const int* n_uniq, int n_uniq_max, const float* uniq_grad, int D,
                                            float grad_scale, const void* step_state, const float* sqnorm, float max_norm, void* stream) {
    AMID_CHECK_ARG(p && m && v && g && n >= 0 && table && m_tab && v_tab && last && uniq_ids && n_uniq && uniq_grad && step_state && D > 0 &&
                   (D % 4) == 0 && n_uniq_max > 0 && sqnorm && max_norm >= 0.0f);
    long long db = (n / 4 + 255) / 256;
    if (db < 1) db = 1;
    if (db > 1024) db = 1024;
    long long rb = ((long long)n_uniq_max + 7) / 8;
    if (rb < 1) rb = 1;
    if (rb > 2048) rb = 2048;
    optimizer_step_clip_kernel<<<(int)(db + rb), 256, 0, (hipStream_t)stream>>>(p, m, v, g, n, (int)db, table, m_tab, v_tab, last, uniq_ids, n_uniq,
                                                                                 uniq_grad, D, (const StepState*)step_state, grad_scale, sqnorm,
                                                                                 max_norm);
    AMID_LAUNCH_CHECK();
    return AMID_OK;
}
