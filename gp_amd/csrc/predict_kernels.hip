// The ends of the GP prediction chains (gpmi_gp_predict, gpmi_seq_marginals; gfx950 only):
//   - the fused row reduction that reads each whitened cross-covariance row T_j = k_j^T L^-T once and leaves the
//     posterior mean T_j . z and variance alpha^2 - T_j . T_j (or, for the sequential sampler, base - T_j . (T B^T)_j);
//   - the backward substitution a = L^-T z of the mean-only path;
//   - the fused build-and-contract kernel mean_j = sum_i k(xs_j, x_i) a_i of that path, which never stores the
//     m x n cross-covariance.
// Reference: what create_p_dotXnS (R/ode_gp_library.R:43-93) returns for its first star point, swept over 41 states at
// R/tests.R:89-97.  Every sum has a fixed shape and order: repeated calls give identical bits.
#include "gpmi_internal.h"
#include "se_device.h"

namespace {

constexpr int PR_SLICE = GPMI_PRED_SLICE, PK_SLICE = GPMI_PRED_KSLICE, PK_SUB = 32, BW = GPMI_PRED_BWD;

// part[(2 slice + 0) mrows + j] = sum over the slice's columns of T[j, c] v[c], part[(2 slice + 1) mrows + j] = the same of
// T[j, c] U[j, c].  thread = row: a wave reads 512 contiguous bytes of each column; four accumulators in a fixed order.
__global__ __launch_bounds__(256) void k_predict_rows_part(const double *T, size_t ldt, const double *U, size_t ldu,
                                                           const double *__restrict__ v, size_t vstride, int n, int mrows,
                                                           double *__restrict__ part)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    const int c0 = blockIdx.y * PR_SLICE;
    const int c1 = (c0 + PR_SLICE < n) ? c0 + PR_SLICE : n;
    if (j >= mrows) return;
    const bool sq = (U == T);   // kernel arguments: uniform
    double am[4] = {0.0, 0.0, 0.0, 0.0}, av[4] = {0.0, 0.0, 0.0, 0.0};
    const double *tc = T + (size_t)j + (size_t)c0 * ldt, *uc = U + (size_t)j + (size_t)c0 * ldu;
    int c = c0;
    for (; c + 4 <= c1; c += 4) {
        double t[4], u[4], w[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            t[q] = tc[(size_t)q * ldt];
            u[q] = sq ? t[q] : uc[(size_t)q * ldu];
            w[q] = v[(size_t)(c + q) * vstride];
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            am[q] = fma(t[q], w[q], am[q]);
            av[q] = fma(t[q], u[q], av[q]);
        }
        tc += 4 * ldt;
        uc += 4 * ldu;
    }
    for (; c < c1; ++c) {
        const double t = tc[0], u = sq ? t : uc[0];
        am[0] = fma(t, v[(size_t)c * vstride], am[0]);
        av[0] = fma(t, u, av[0]);
        tc += ldt;
        uc += ldu;
    }
    part[((size_t)2 * blockIdx.y + 0) * mrows + j] = (am[0] + am[1]) + (am[2] + am[3]);
    part[((size_t)2 * blockIdx.y + 1) * mrows + j] = (av[0] + av[1]) + (av[2] + av[3]);
}

// the slice sums in slice order; a non-zero factorisation status turns every output into NaN
__global__ __launch_bounds__(256) void k_predict_rows_sum(const double *__restrict__ part, int nslice, int mrows, double base,
                                                          double *__restrict__ mean, double *__restrict__ var, const int *info,
                                                          int *info_out)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    const int bad = info ? *info : 0;
    if (info_out && j == 0) *info_out = bad;
    if (j >= mrows) return;
    double sm = 0.0, sv = 0.0;
    for (int q = 0; q < nslice; ++q) {
        sm += part[((size_t)2 * q + 0) * mrows + j];
        sv += part[((size_t)2 * q + 1) * mrows + j];
    }
    mean[j] = bad ? __builtin_nan("") : sm;
    if (var) var[j] = bad ? __builtin_nan("") : base - sv;
}

// One block of the backward substitution a = L^-T z, blocks taken last to first.  EVERY workgroup solves the diagonal block
// L_kk^T a_k = z_k itself (one wave, the 64 x 64 block in LDS, column-oriented: the same instructions on the same numbers in every
// workgroup, so all of them hold the same a_k; workgroup 0 stores it), then takes a_k out of its share of the entries in front:
// z[i] -= sum_r L[k0 + r, i] a_k[r], one wave per column (its 64 rows are one 512-byte line), summed by a butterfly of fixed shape.
// z[k0 .. k0 + kb) is only read and z[0 .. k0) only written by this launch.
__global__ __launch_bounds__(256) void k_trsv_t_block(const double *__restrict__ L, size_t ldl, int k0, int kb, double *z,
                                                      double *__restrict__ a)
{
    __shared__ double s_L[BW][BW + 1];
    __shared__ double s_a[BW];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int e = tid; e < BW * BW; e += 256) {
        const int r = e & (BW - 1), c = e / BW;
        s_L[r][c] = (r < kb && c <= r) ? L[(size_t)(k0 + r) + (size_t)(k0 + c) * ldl] : (r == c ? 1.0 : 0.0);
    }
    __syncthreads();
    if (wave == 0) {
        double b = lane < kb ? z[k0 + lane] : 0.0;
        for (int j = BW - 1; j >= 0; --j) {
            const double aj = __shfl(b, j) / s_L[j][j];
            if (lane == j) b = aj;
            else if (lane < j) b = fma(-s_L[j][lane], aj, b);
        }
        s_a[lane] = b;
        if (blockIdx.x == 0 && lane < kb) a[k0 + lane] = b;
    }
    __syncthreads();
    const double al = s_a[lane];
    const int i0 = blockIdx.x * 32 + wave * 8;
    double v[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const int i = i0 + q;
        v[q] = (i < k0 && lane < kb) ? L[(size_t)(k0 + lane) + (size_t)i * ldl] * al : 0.0;
    }
#pragma unroll
    for (int q = 0; q < 8; ++q) {
#pragma unroll
        for (int h = 32; h > 0; h >>= 1) v[q] += __shfl_xor(v[q], h);
    }
    if (lane == 0) {
#pragma unroll
        for (int q = 0; q < 8; ++q)
            if (i0 + q < k0) z[i0 + q] -= v[q];
    }
}

// part[slice m + j] = sum over the slice's PK_SLICE training points of k(xs_j, x_i) a_i.  thread = test point, a workgroup owns
// 256 of them; the slice streams through LDS in sub-slices of PK_SUB points (scaled coordinates and a).  Per sub-slice the
// thread keeps PK_SUB squared distances in registers and walks the dimensions outermost -- d ascending, one subtraction and
// one fma per pair and dimension, exactly se_cov_tile's order -- so D needs no register file of its own: DT = 1..3 keep the test
// point's coordinates in registers, DT = 0 (any D <= 64) re-reads them from the (cached) input.  n m exponentials: the kernel is
// bound by them, not by memory.
template <int DT>
__global__ __launch_bounds__(256) void k_predict_mean_part(const double *__restrict__ X, int n, int ldx, const double *__restrict__ Xs,
                                                           int m, int ldxs, SeParams p, const double *__restrict__ a,
                                                           double *__restrict__ part, ExpC ec)
{
    __shared__ double s_x[GPMI_MAXD_BIG][PK_SUB];
    __shared__ double s_a[PK_SUB];
    const int D = DT > 0 ? DT : p.D;
    const int tid = threadIdx.x;
    const int j = blockIdx.x * 256 + tid, jc = j < m ? j : m - 1;
    const int i0 = blockIdx.y * PK_SLICE;
    double xr[DT > 0 ? DT : 1];
    if (DT > 0) {
#pragma unroll
        for (int d = 0; d < DT; ++d) xr[d] = __dmul_rn(Xs[(size_t)jc + (size_t)d * ldxs], p.inv_ell[d]);
    }
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int s0 = i0; s0 < i0 + PK_SLICE && s0 < n; s0 += PK_SUB) {
        __syncthreads();
        for (int e = tid; e < D * PK_SUB; e += 256) {
            const int d = e / PK_SUB, q = e - d * PK_SUB, i = s0 + q;
            s_x[d][q] = i < n ? __dmul_rn(X[(size_t)i + (size_t)d * ldx], p.inv_ell[d]) : 0.0;
        }
        if (tid < PK_SUB) s_a[tid] = (s0 + tid < n) ? a[s0 + tid] : 0.0;
        __syncthreads();
        double s[PK_SUB];
#pragma unroll
        for (int q = 0; q < PK_SUB; ++q) s[q] = 0.0;
        if (DT > 0) {
#pragma unroll
            for (int d = 0; d < DT; ++d) {
#pragma unroll
                for (int q = 0; q < PK_SUB; ++q) {
                    const double df = __dsub_rn(xr[d], s_x[d][q]);
                    s[q] = fma(df, df, s[q]);
                }
            }
        } else {
            for (int d = 0; d < D; ++d) {
                const double xd = __dmul_rn(Xs[(size_t)jc + (size_t)d * ldxs], p.inv_ell[d]);
#pragma unroll
                for (int q = 0; q < PK_SUB; ++q) {
                    const double df = __dsub_rn(xd, s_x[d][q]);
                    s[q] = fma(df, df, s[q]);
                }
            }
        }
#pragma unroll
        for (int q = 0; q < PK_SUB; ++q) {
            const double kv = p.a2 * exp_nonpos(-0.5 * s[q], ec);
            acc[q & 3] = fma(kv, s_a[q], acc[q & 3]);
        }
    }
    if (j < m) part[(size_t)blockIdx.y * m + j] = (acc[0] + acc[1]) + (acc[2] + acc[3]);
}

__global__ __launch_bounds__(256) void k_predict_mean_sum(const double *__restrict__ part, int nslice, int m, double *__restrict__ mean,
                                                          const int *info, int *info_out)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    const int bad = info ? *info : 0;
    if (info_out && j == 0) *info_out = bad;
    if (j >= m) return;
    double sm = 0.0;
    for (int q = 0; q < nslice; ++q) sm += part[(size_t)q * m + j];
    mean[j] = bad ? __builtin_nan("") : sm;
}

}  // namespace

size_t predict_rows_part_doubles(int n, int mrows)
{
    return (size_t)2 * (size_t)((n + PR_SLICE - 1) / PR_SLICE) * (size_t)mrows;
}

size_t predict_mean_part_doubles(int n, int m)
{
    return (size_t)((n + PK_SLICE - 1) / PK_SLICE) * (size_t)m;
}

void launch_predict_rows(hipStream_t s, const double *T, size_t ldt, const double *U, size_t ldu, const double *v, size_t vstride,
                         int n, int mrows, double base, double *part, double *mean, double *var, const int *info, int *info_out)
{
    if (n <= 0 || mrows <= 0) return;
    const int nslice = (n + PR_SLICE - 1) / PR_SLICE;
    hipLaunchKernelGGL(k_predict_rows_part, dim3((mrows + 255) / 256, nslice), 256, 0, s, T, ldt, U, ldu, v, vstride, n, mrows, part);
    hipLaunchKernelGGL(k_predict_rows_sum, dim3((mrows + 255) / 256), 256, 0, s, part, nslice, mrows, base, mean, var, info, info_out);
}

void launch_trsv_lower_t(hipStream_t s, const double *L, size_t ldl, int n, double *z, double *a)
{
    if (n <= 0) return;
    for (int k0 = ((n - 1) / BW) * BW; k0 >= 0; k0 -= BW) {
        const int kb = (n - k0 < BW) ? n - k0 : BW;
        const int wg = k0 > 0 ? (k0 + 31) / 32 : 1;
        hipLaunchKernelGGL(k_trsv_t_block, dim3(wg), 256, 0, s, L, ldl, k0, kb, z, a);
    }
}

void launch_predict_mean(hipStream_t s, const double *X, int n, int ldx, const double *Xs, int m, int ldxs, const SeParams &p,
                         const double *a, double *part, double *mean, const int *info, int *info_out)
{
    if (n <= 0 || m <= 0) return;
    const int nslice = (n + PK_SLICE - 1) / PK_SLICE;
    const dim3 grid((m + 255) / 256, nslice);
    switch (p.D) {
    case 1: hipLaunchKernelGGL(k_predict_mean_part<1>, grid, 256, 0, s, X, n, ldx, Xs, m, ldxs, p, a, part, h_exp); break;
    case 2: hipLaunchKernelGGL(k_predict_mean_part<2>, grid, 256, 0, s, X, n, ldx, Xs, m, ldxs, p, a, part, h_exp); break;
    case 3: hipLaunchKernelGGL(k_predict_mean_part<3>, grid, 256, 0, s, X, n, ldx, Xs, m, ldxs, p, a, part, h_exp); break;
    default: hipLaunchKernelGGL(k_predict_mean_part<0>, grid, 256, 0, s, X, n, ldx, Xs, m, ldxs, p, a, part, h_exp); break;
    }
    hipLaunchKernelGGL(k_predict_mean_sum, dim3((m + 255) / 256), 256, 0, s, part, nslice, m, mean, info, info_out);
}
