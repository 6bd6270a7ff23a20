// Gradient clipping for the optimizer of the reference's own loop (amid_amd/optim.py): torch.nn.utils.clip_grad_norm_ over EVERY parameter,
// the item table included, without ever forming the table's dense gradient.
//   amid_grad_sqnorm_f32          sum of g^2 over the flat dense gradient and the step's segment-reduced unique rows [0, *n_uniq)
// The clipped step itself is amid_optimizer_step_clip_f32 (adam.hip): amid_optimizer_step_f32 whose gradients are scaled by grad_scale * c,
// c = min(1, max_norm / (sqrt(*sqnorm) + 1e-6)): torch's clip coefficient, read on the device.
// The norm is two small launches, not one with a last-block finish: 1.7 MB + a few thousand 512-byte rows is latency-bound either way, the
// finish of a one-launch form needs a ticket that somebody has to zero (a workspace with state), and the second launch is 256 doubles.  The
// sum is taken in double in a fixed order -- thread-sequential, wave shuffles, LDS across waves, then one block over the partials -- with a
// grid that does not depend on the data: no float atomics, the same bits on every run.
#include "common.h"

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
