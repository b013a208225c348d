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

// ---- the ends of the joint posterior's chain (gpmi_gp_predict_joint) -------------------------------------------------
// After the augmented partial factorisation the workspace holds the Schur block S (m x m, lower) and, in the row below it,
// -mean^T.  mean[r] = -row[r] and S[r, r] += post_jitter (thread = r: the only writer of that element) ...
// pj: one post_jitter per block of mb rows (gpmi_joint_predict: a block per derivative order); gpmi_gp_predict_joint has one block
struct BlockJitter {
    double v[3];
    int mb;
};
__global__ __launch_bounds__(256) void k_joint_mean_diag(double *__restrict__ S, size_t ld, const double *__restrict__ row, int m,
                                                         BlockJitter pj, double *__restrict__ mean, const int *info)
{
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= m) return;
    mean[r] = *info ? __builtin_nan("") : -row[(size_t)r * ld];
    S[(size_t)r * (ld + 1)] += r < pj.mb ? pj.v[0] : (r < 2 * pj.mb ? pj.v[1] : pj.v[2]);
}

// ... then cov = S mirrored (both triangles from the SAME stored element: bit-for-bit symmetric), NaN when *info != 0.
// thread = row, 64 rows x 16 columns per workgroup; the upper half reads S along its columns as well (the element (c, r))
__global__ __launch_bounds__(256) void k_joint_cov(const double *__restrict__ S, size_t ld, int m, double *__restrict__ cov, size_t ldc,
                                                   const int *info)
{
    __shared__ double s_t[16][65];
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int r0 = blockIdx.x * 64, c0 = blockIdx.y * 16;
    const int bad = *info;
    // upper part of this block (r < c): the 16 x 64 piece S[c0 .. c0 + 16, r0 .. r0 + 64) read with the lanes along its rows c
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int e = q * 256 + (int)threadIdx.x, cc = e & 15, rr = e >> 4;
        const int c = c0 + cc, r = r0 + rr;
        s_t[cc][rr] = (c < m && r < c) ? S[(size_t)c + (size_t)r * ld] : 0.0;
    }
    __syncthreads();
    const int r = r0 + tx;
    if (r >= m) return;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int cc = ty * 4 + q, c = c0 + cc;
        if (c < m) {
            const double v = (r >= c) ? S[(size_t)r + (size_t)c * ld] : s_t[cc][tx];
            cov[(size_t)r + (size_t)c * ldc] = bad ? __builtin_nan("") : v;
        }
    }
}

// Draws = mean 1^T + Lc Z: Lc m x m lower (leading dimension ldl; whatever lies above its diagonal is never used), Z and
// Draws m x B.  A lower-triangular matrix-matrix product on v_mfma_f64_16x16x4_f64 with the operand conventions of gemm_tile
// (gpmi_probe_mfma): lane l gives A[row l & 15][k l >> 4] and B[k l >> 4][col l & 15] and receives D[row (l >> 4) + 4 i][col l & 15]
// in element i.  A workgroup owns TD_R = 64 rows (wave w rows 16 w .. 16 w + 15) and up to 64 columns (four accumulator tiles
// per wave) and walks k in chunks of TD_K = 32 from 0 to the end of its diagonal tile: the chunk of Lc (64 x 32, elements with
// k > row and rows >= m replaced by exact zeros) and of Z (32 x 64, zeros past m and B) are loaded into registers one chunk
// ahead of the MFMAs and passed through LDS.  Lc is therefore read once per 64 columns of Z (launch_trmv_lower: once per column).
// LDS images (ds_read_b64 serves 32 lanes per pass, 64 banks of 4 bytes):
//   s_a[k][row], stride 80 doubles: a pass reads rows lr = 0..15 of k and k + 1: 160 dwords apart = 32 banks -> all 64 distinct;
//   s_z[col][k], stride 34 doubles: a pass reads columns lr = 0..15 (68 dwords apart = 4 banks) at k, k + 1 (2 dwords) -> distinct.
// Every output element is one accumulator element summed over k = 0, 1, 2, ... in chunks that depend on its row tile alone:
// column b has the same bits whatever B is and whatever the other columns hold.  The tile is written out through LDS so that
// the stores run along the columns of Draws.  info_a / info_b (device; info_b nullable): non-zero -> every draw is NaN.
constexpr int TD_R = 64, TD_K = 32, TD_C = 64, TD_SA = 80, TD_SZ = 34, TD_SO = 66;
__global__ __launch_bounds__(256) void k_tril_draws(const double *__restrict__ L, size_t ldl, int m, const double *__restrict__ mean,
                                                    const double *__restrict__ Z, size_t ldz, int B, double *__restrict__ draws,
                                                    size_t ldd, const int *info_a, const int *info_b)
{
    static_assert(TD_K * TD_SA + TD_C * TD_SZ >= TD_C * TD_SO, "the output tile reuses the operand images");
    __shared__ double s_buf[TD_K * TD_SA + TD_C * TD_SZ];
    double *s_a = s_buf, *s_z = s_buf + TD_K * TD_SA;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, lr = lane & 15, lq = lane >> 4;
    const int i0 = ((int)gridDim.x - 1 - (int)blockIdx.x) * TD_R;   // the long row tiles start first
    const int c0 = blockIdx.y * TD_C;
    const int kend = i0 + TD_R < m ? i0 + TD_R : m;
    const int nch = (kend + TD_K - 1) / TD_K;
    const int nct = (B - c0 + 15) / 16 < 4 ? (B - c0 + 15) / 16 : 4;   // column tiles in use (workgroup-uniform)
    const int gr = i0 + lane;                       // staging of Lc: row `lane`, k = w + 4 j
    const int zk = tid & (TD_K - 1), zc = tid >> 5;  // staging of Z: k = zk, column zc + 8 j
    double pa[8], pz[8];
    auto gload = [&](int k0) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int gk = k0 + w + 4 * j;
            pa[j] = (gr < m && gk <= gr) ? L[(size_t)gr + (size_t)gk * ldl] : 0.0;
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int gk = k0 + zk, gc = c0 + zc + 8 * j;
            pz[j] = (gk < m && gc < B) ? Z[(size_t)gk + (size_t)gc * ldz] : 0.0;
        }
    };
    d4 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = d4{0.0, 0.0, 0.0, 0.0};
    gload(0);
    for (int ch = 0; ch < nch; ++ch) {
        __syncthreads();   // the previous chunk's fragments have been read
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            s_a[(w + 4 * j) * TD_SA + lane] = pa[j];
            s_z[(zc + 8 * j) * TD_SZ + zk] = pz[j];
        }
        __syncthreads();
        if (ch + 1 < nch) gload((ch + 1) * TD_K);
#pragma unroll
        for (int kk = 0; kk < TD_K / 4; ++kk) {
            const double a = s_a[(4 * kk + lq) * TD_SA + 16 * w + lr];
#pragma unroll
            for (int t = 0; t < 4; ++t)
                if (t < nct) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, s_z[(16 * t + lr) * TD_SZ + 4 * kk + lq], acc[t], 0, 0, 0);
        }
    }
    __syncthreads();
    double *s_o = s_buf;   // [column][row], stride TD_SO
#pragma unroll
    for (int t = 0; t < 4; ++t)
        if (t < nct) {
#pragma unroll
            for (int i = 0; i < 4; ++i) s_o[(16 * t + lr) * TD_SO + 16 * w + lq + 4 * i] = acc[t][i];
        }
    __syncthreads();
    const int bad = *info_a | (info_b ? *info_b : 0);
    if (gr < m) {
        const double mu = mean[gr];
        for (int col = w; col < 16 * nct; col += 4) {
            const int gc = c0 + col;
            if (gc < B) draws[(size_t)gr + (size_t)gc * ldd] = bad ? __builtin_nan("") : s_o[col * TD_SO + lane] + mu;
        }
    }
}

}  // namespace

void launch_joint_readout_blocks(hipStream_t s, double *S, size_t ld, const double *row, int m, const double *pj, int mb, double *mean,
                                 double *cov, size_t ldc, const int *info)
{
    if (m <= 0) return;
    const BlockJitter bj = {{pj[0], m > mb ? pj[1] : 0.0, m > 2 * mb ? pj[2] : 0.0}, mb};
    hipLaunchKernelGGL(k_joint_mean_diag, dim3((m + 255) / 256), 256, 0, s, S, ld, row, m, bj, mean, info);
    if (cov) hipLaunchKernelGGL(k_joint_cov, dim3((m + 63) / 64, (m + 15) / 16), 256, 0, s, S, ld, m, cov, ldc, info);
}

void launch_joint_readout(hipStream_t s, double *S, size_t ld, const double *row, int m, double post_jitter, double *mean, double *cov,
                          size_t ldc, const int *info)
{
    launch_joint_readout_blocks(s, S, ld, row, m, &post_jitter, m, mean, cov, ldc, info);   // one block: the same one addition
}

void launch_tril_draws(hipStream_t s, const double *L, size_t ldl, int m, const double *mean, const double *Z, size_t ldz, int B,
                       double *draws, size_t ldd, const int *info_a, const int *info_b)
{
    if (m <= 0 || B <= 0) return;
    hipLaunchKernelGGL(k_tril_draws, dim3((m + TD_R - 1) / TD_R, (B + TD_C - 1) / TD_C), 256, 0, s, L, ldl, m, mean, Z, ldz, B, draws,
                       ldd, info_a, info_b);
}

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
