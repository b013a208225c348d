// Exact leave-one-out cross-validation of the GP (gpmi_logml_loo; Rasmussen & Williams 5.4.2; gfx950 only): the O(n^2)
// passes between the factorisation chain, which leaves -A = -S^-1 (lower triangle) and a = S^-1 y on the device, and the
// gradient contraction.  With d = diag A:
//   mu_i = y_i - a_i / d_i,  var_i = 1 / d_i,  lpd_i = -1/2 log(2 pi) + 1/2 log d_i - a_i^2 / (2 d_i),  loo = sum_i lpd_i,
//   d loo / d theta = sum_kl G_kl dS_kl / d theta,  G = (b a' + a b') / 2 - A diag(v) A,
//   u_i = a_i / d_i,  v_i = (1 + a_i^2 / d_i) / (2 d_i) > 0,  b = A u.
// A diag(v) A = M M' with M = A diag(sqrt v) is one symmetric rank-n product (the trailing-update SYRK); here are the point
// kernel, the tile pass that writes M and b, and the finishing kernel.  Every sum has a fixed shape and order: no atomics,
// repeated calls give identical bits.
#include "gpmi_internal.h"

namespace {

constexpr int LOO_PITCH = 65;   // row pitch of the 64 x 64 tile in LDS: column-wise writes and transposed reads without bank conflicts

// One workgroup.  d_i = -Wk[i, i] (Wk: the lower triangle of -A), a_i = asign av_i (the augmented chain hands over -a).
// mu, var, lpd are nullable; ab[0 .. n) = a, u, sv = sqrt(v) always.  *loo = the lpd_i summed per thread in index order
// (stride 1024), then one tree over the 1024 threads.  *info != 0 (not positive definite): NaN to every output.
__global__ __launch_bounds__(1024) void k_loo_points(const double *__restrict__ Wk, size_t ld, int n, const double *__restrict__ av,
                                                     double asign, const double *__restrict__ y, const int *__restrict__ info,
                                                     double *__restrict__ mu, double *__restrict__ var, double *__restrict__ lpd,
                                                     double *__restrict__ ab, double *__restrict__ u, double *__restrict__ sv,
                                                     double *__restrict__ loo)
{
    __shared__ double red[1024];
    const bool bad = *info != 0;
    const double nan = __builtin_nan("");
    double acc = 0.0;
    for (int i = threadIdx.x; i < n; i += 1024) {
        const double d = -Wk[(size_t)i + (size_t)i * ld], a = asign * av[i];
        const double ui = a / d, q = a * ui;   // a_i^2 / d_i
        const double l = -0.91893853320467274178 + 0.5 * log(d) - 0.5 * q;
        ab[i] = a;
        u[i] = ui;
        sv[i] = sqrt(0.5 * (1.0 + q) / d);
        if (mu) mu[i] = bad ? nan : y[i] - ui;
        if (var) var[i] = bad ? nan : 1.0 / d;
        if (lpd) lpd[i] = bad ? nan : l;
        acc += l;
    }
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int h = 512; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x == 0) *loo = bad ? nan : red[0];
}

// One 64 x 64 tile (ti, tj), tj <= ti, of the lower triangle of Wk = -A; thread = one row x 16 columns.  The tile goes through
// LDS (read along columns); the tile above the diagonal is the transposed tile, so the stores of both run along columns too.
//   M[i, j] = A_ij sv_j for the tile and its mirror image (both triangles of M are written);
//   bpart[tj][64 ti + r] = sum_{j in tile} A_ij u_j (row part), and off the diagonal bpart[ti][64 tj + r] = sum_{i in tile} A_ij u_i
//   (transposed part): slot t of row block R is written once, by tile (R, t) for t <= R and by tile (t, R) for t > R.
// The 16 terms of a thread are added in column order, the four threads of a row in a fixed order.
__global__ __launch_bounds__(256) void k_loo_tiles(const double *__restrict__ Wk, size_t ld, int n, const double *__restrict__ u,
                                                   const double *__restrict__ sv, double *__restrict__ M, size_t ldm,
                                                   double *__restrict__ bpart)
{
    __shared__ double sa[64 * LOO_PITCH], su[2][64], ss[2][64], rs[2][4][64];
    const int ti = blockIdx.x, tj = blockIdx.y;
    if (tj > ti) return;
    const int lane = threadIdx.x & 63, grp = threadIdx.x >> 6;
    const bool diag = ti == tj;
    const size_t npad = (size_t)gridDim.x * 64;
    {   // sa[c][r] = A[64 ti + r, 64 tj + c] where the lower triangle holds it, 0 elsewhere
        const int i = ti * 64 + lane;
        for (int cc = grp; cc < 64; cc += 4) {
            const int j = tj * 64 + cc;
            sa[cc * LOO_PITCH + lane] = (i < n && j < n && j <= i) ? -Wk[(size_t)i + (size_t)j * ld] : 0.0;
        }
        if (grp < 2) {   // u and sqrt(v) of the tile's columns [0] and rows [1]
            const int k = (grp ? ti : tj) * 64 + lane;
            su[grp][lane] = k < n ? u[k] : 0.0;
            ss[grp][lane] = k < n ? sv[k] : 0.0;
        }
    }
    __syncthreads();
    double racc = 0.0, cacc = 0.0;
    {
        const int i = ti * 64 + lane;
        for (int q = 0; q < 16; ++q) {
            const int c = grp * 16 + q, j = tj * 64 + c;
            const double v = (diag && c > lane) ? sa[lane * LOO_PITCH + c] : sa[c * LOO_PITCH + lane];
            if (i < n && j < n) M[(size_t)i + (size_t)j * ldm] = v * ss[0][c];
            racc += v * su[0][c];
        }
    }
    if (!diag) {
        const int j = tj * 64 + lane;   // row of the mirror tile
        for (int q = 0; q < 16; ++q) {
            const int r = grp * 16 + q, i = ti * 64 + r;
            const double v = sa[lane * LOO_PITCH + r];
            if (i < n && j < n) M[(size_t)j + (size_t)i * ldm] = v * ss[1][r];
            cacc += v * su[1][r];
        }
    }
    rs[0][grp][lane] = racc;
    rs[1][grp][lane] = cacc;
    __syncthreads();
    if (grp == 0)
        bpart[(size_t)tj * npad + (size_t)ti * 64 + lane] = (rs[0][0][lane] + rs[0][1][lane]) + (rs[0][2][lane] + rs[0][3][lane]);
    else if (grp == 1 && !diag)
        bpart[(size_t)ti * npad + (size_t)tj * 64 + lane] = (rs[1][0][lane] + rs[1][1][lane]) + (rs[1][2][lane] + rs[1][3][lane]);
}

// b_i = the T slots of row i added in slot order
__global__ __launch_bounds__(256) void k_loo_bsum(const double *__restrict__ bpart, int T, int n, double *__restrict__ b)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const size_t npad = (size_t)T * 64;
    double acc = 0.0;
    for (int t = 0; t < T; ++t) acc += bpart[(size_t)t * npad + i];
    b[i] = acc;
}

// grad = (d/dalpha, d/dell..., d/dsigma) from the contraction sums (the statements of gpmi_logml_grad's finish), NaN when
// *info != 0
__global__ void k_loo_grad_finish(const double *__restrict__ sums, int D, int ns, double alpha, GradEll e, int n_ell, double sigma,
                                  const int *__restrict__ info, double *__restrict__ grad)
{
    if (threadIdx.x != 0) return;
    if (*info != 0) {
        for (int k = 0; k < 2 + n_ell; ++k) grad[k] = __builtin_nan("");
    } else {
        gpmi_grad_from_sums(sums, D, alpha, e.ell, n_ell, grad);
        grad[1 + n_ell] = 2.0 * sigma * sums[ns - 1];
    }
}

}  // namespace

size_t loo_bpart_doubles(int n)
{
    const size_t T = (size_t)((n + 63) / 64);
    return T * T * 64;
}

void launch_loo_points(hipStream_t s, const double *Wk, size_t ld, int n, const double *av, double asign, const double *y,
                       const int *info, double *mu, double *var, double *lpd, double *ab, double *u, double *sv, double *loo)
{
    hipLaunchKernelGGL(k_loo_points, dim3(1), 1024, 0, s, Wk, ld, n, av, asign, y, info, mu, var, lpd, ab, u, sv, loo);
}

void launch_loo_tiles(hipStream_t s, const double *Wk, size_t ld, int n, const double *u, const double *sv, double *M, size_t ldm,
                      double *bpart, double *b)
{
    const int T = (n + 63) / 64;
    hipLaunchKernelGGL(k_loo_tiles, dim3(T, T), 256, 0, s, Wk, ld, n, u, sv, M, ldm, bpart);
    hipLaunchKernelGGL(k_loo_bsum, dim3((n + 255) / 256), 256, 0, s, bpart, T, n, b);
}

void launch_loo_grad_finish(hipStream_t s, const double *sums, int D, int ns, double alpha, const double *ell, int n_ell, double sigma,
                            const int *info, double *grad)
{
    hipLaunchKernelGGL(k_loo_grad_finish, dim3(1), 64, 0, s, sums, D, ns, alpha, grad_ell(ell, n_ell), n_ell, sigma, info, grad);
}
