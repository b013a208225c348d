// The likelihood head of the blocked chain of gpmi_latent_gp_lp_grad (n > 256, e.g. models/westbrook_exact.stan at N = 1438):
// between F = L Z and Zbar = L^T Fbar, one pass over F (n x k) and Y (n x m) writes Fbar and one partial (lik, d lik / d sigma)
// pair per block of 256 rows; a one-block kernel adds the partials in index order.  No atomics and no counters: repeated calls
// give identical bits.  O(n m) against the chain's O(n^3): coalesced column-major reads (thread = row) are all it needs.
#include "gpmi_internal.h"

namespace {
#include "latent_device.h"

__global__ __launch_bounds__(256) void k_latent_head(const double *__restrict__ F, size_t ldf, int n, int k, LatentHead lh,
                                                     double *__restrict__ Fb, size_t ldfb, double *__restrict__ part)
{
    __shared__ double s_r[8];
    const int tid = threadIdx.x, i = blockIdx.x * 256 + tid;
    double red[2] = {0.0, 0.0}, fb[2] = {0.0, 0.0};
    if (i < n) {
        const double f0 = F[i], f1 = k > 1 ? F[(size_t)i + ldf] : 0.0;
        latent_head_row(lh, f0, f1, lh.Y + i, red[0], red[1], fb[0], fb[1]);
        Fb[i] = fb[0];
        if (k > 1) Fb[(size_t)i + ldfb] = fb[1];
    }
    // butterfly inside every wave, the four wave sums in wave order (as the one-workgroup kernel)
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        double v = red[q];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
        if ((tid & 63) == 0) s_r[(tid >> 6) * 2 + q] = v;
    }
    __syncthreads();
    if (tid < 2) part[2 * (size_t)blockIdx.x + tid] = ((s_r[tid] + s_r[2 + tid]) + s_r[4 + tid]) + s_r[6 + tid];
}

// out[0..1] = the partial pairs added in block order; not positive definite: NaN there and in Fbar
__global__ __launch_bounds__(256) void k_latent_head_sum(const double *__restrict__ part, int nblk, double *__restrict__ out,
                                                         double *__restrict__ Fb, size_t ldfb, int n, int k, const int *__restrict__ info)
{
    const int tid = threadIdx.x;
    const bool bad = *info != 0;
    if (tid < 2) {
        double t = 0.0;
        for (int b = 0; b < nblk; ++b) t += part[2 * (size_t)b + tid];
        out[tid] = bad ? __builtin_nan("") : t;
    }
    if (bad)
        for (int c = 0; c < k; ++c)
            for (int i = tid; i < n; i += 256) Fb[(size_t)i + (size_t)c * ldfb] = __builtin_nan("");
}
}  // namespace

int latent_head_blocks(int n) { return (n + 255) / 256; }

void launch_latent_head(hipStream_t s, const double *F, size_t ldf, int n, int k, const LatentHead &lh, double *Fb, size_t ldfb,
                        double *part, double *out, const int *info)
{
    const int nblk = latent_head_blocks(n);
    hipLaunchKernelGGL(k_latent_head, dim3(nblk), 256, 0, s, F, ldf, n, k, lh, Fb, ldfb, part);
    hipLaunchKernelGGL(k_latent_head_sum, dim3(1), 256, 0, s, part, nblk, out, Fb, ldfb, n, k, info);
}
