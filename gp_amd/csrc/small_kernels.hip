// One-workgroup ("small-N") kernels and their launchers: a whole evaluation -- covariance build, factorisation, solves,
// reductions -- by ONE workgroup of one launch, on the device functions of the blocked Cholesky (chol_device.h).  The
// section comment below states the scheme; chol_kernels.hip holds the blocked kernels and the launch chains.
#include "chol_device.h"

namespace {

#include "se_device.h"
#include "latent_device.h"


// ---------------------------------------------------------------------------
// Small problems: ONE workgroup does a whole evaluation.
//
// The reference's drivers call the path at N = 21 (R/tests.R:5-19), 79 .. 199 (pendulum_fit*.R:206-214) and
// 256 (BASELINE c1); there the chain of launches of the blocked code (build, row, diagonal block, panel solve,
// update, ..., two finalize kernels) is pure launch latency.  Here one workgroup of 4 waves runs the same
// device functions back to back on a matrix that never leaves its CU's L2:
//   build (se_cov_tile: the arithmetic of k_se_cov, bit-identical K)  ->  for every 128-column panel:
//   potrf_diag4_body (packed factors to LDS)  ->  rows below by trsm_panel_body strips  ->  trailing tiles by
//   gemm_tile<1> / gemm_quad64  ->  log-det and quadratic form, reduced in the order of k_logml_partial.
// The right-hand side y rides along as row n; when it is the only row below the last panel
// its solve is a VALU forward substitution from the packed factors in LDS (two barriers per 16 pivots) instead
// of a 144-MFMA strip.  Phase boundaries are __syncthreads(): global memory written by one wave of a workgroup
// is visible to the others behind the barrier (one CU, one L1).  A grid of G hyper-parameter points is G
// workgroups of ONE launch (k_logml_small_batch), each with its own workspace slice.
// ---------------------------------------------------------------------------
#ifdef GPMI_PROBES  // phase stamps of the small kernels (block 0, thread 0): g_small[0] build, [1] diagonal blocks, [2] rows below, [3] launches, [4] trailing tiles, [5] finalize
__device__ unsigned long long g_small[8];  // this translation unit's own array: without relocatable device code none can be shared with chol_kernels.hip
#define GPMI_STAMP(v) const unsigned long long v = __builtin_amdgcn_s_memtime();
#define GPMI_STAMP_ADD(i, d) if (threadIdx.x == 0 && blockIdx.x == 0) atomicAdd(&g_small[i], (unsigned long long)(d));
#else
#define GPMI_STAMP(v)
#define GPMI_STAMP_ADD(i, d)
#endif
struct SmallSe {            // hyper-parameters of one point, in registers
    double a2;
    double inv_ell[GPMI_MAXD];
    int D;
};

// ---- steps every one-workgroup kernel shares: each stated once ---------------------------------------------
// (plain pointers, no __restrict__: after inlining the kernels' own argument attributes are what the optimiser sees, as
// they were when these loops stood in the kernels)

// hyper-parameters of one point into registers: a length-scale per dimension (kernel argument or device memory) ...
__device__ __forceinline__ SmallSe small_se(double a2, const double *inv_ell, int D)
{
    SmallSe se;
    se.a2 = a2;
    se.D = D;
#pragma unroll
    for (int d = 0; d < GPMI_MAXD; ++d) se.inv_ell[d] = inv_ell[d];
    return se;
}
// ... or one for all
__device__ __forceinline__ SmallSe small_se_iso(double a2, double inv_rho, int D)
{
    SmallSe se;
    se.a2 = a2;
    se.D = D;
#pragma unroll
    for (int d = 0; d < GPMI_MAXD; ++d) se.inv_ell[d] = inv_rho;
    return se;
}

// Host-mapped inputs (the host-buffer entry points): ONE coalesced pass with every load in flight (one PCIe round trip)
// into `stage` in device memory -- X (n x D, ldx) first, then the columns of A (ka, lda) and of B (kb, ldb), every block
// packed with leading dimension n.  The host sizes the buffer from this order.  Ends with the workgroup's barrier.
__device__ __forceinline__ void small_stage(double *stage, int n, int tid, const double *X, int D, int ldx, const double *A, int ka,
                                            int lda, const double *B = nullptr, int kb = 0, int ldb = 0)
{
    const int nx = n * D, na = n * ka, nb = n * kb;
    for (int e = tid; e < nx + na + nb; e += 256) {
        if (e < nx) {
            const int d = e / n, i = e - d * n;
            stage[e] = X[(size_t)i + (size_t)d * ldx];
        } else if (e < nx + na) {
            const int c = (e - nx) / n, i = e - nx - c * n;
            stage[e] = A[(size_t)i + (size_t)c * lda];
        } else {
            const int c = (e - nx - na) / n, i = e - nx - na - c * n;
            stage[e] = B[(size_t)i + (size_t)c * ldb];
        }
    }
    __syncthreads();
}

// scaled coordinates x_id / ell_d of n points, dimension-major with stride n, into LDS: for the covariance build (the
// staging buffer of the later phases is free then: one global round trip instead of one per tile and operand) and,
// after the factorisation, for the contractions of the gradient kernels.  No barrier: the callers differ about it.
__device__ __forceinline__ void small_scale_x(double *xs, const double *X, int n, int ldx, const SmallSe &se, int tid)
{
#pragma unroll
    for (int d = 0; d < GPMI_MAXD; ++d)
        if (d < se.D)
            for (int i = tid; i < n; i += 256) xs[i + d * n] = __dmul_rn(X[(size_t)i + (size_t)d * ldx], se.inv_ell[d]);
}

// covariance of nt points from their scaled coordinates in LDS, lower SE_TR x SE_TC tiles (se_cov_tile: the arithmetic of
// k_se_cov, bit-identical K), diag_add on the diagonal
__device__ __forceinline__ void small_se_build(const double *xs, int nt, const SmallSe &se, double diag_add, double *W, size_t ld,
                                               const ExpC &ec)
{
    for (int row0 = 0; row0 < nt; row0 += SE_TR)
        for (int col0 = 0; col0 < row0 + SE_TR && col0 < nt; col0 += SE_TC) {
            switch (se.D) {
            case 1: se_cov_tile<1, true>(xs, nt, nt, xs, nt, nt, se, diag_add, 1, 1, W, ld, 1, ec, row0, col0); break;
            case 2: se_cov_tile<2, true>(xs, nt, nt, xs, nt, nt, se, diag_add, 1, 1, W, ld, 1, ec, row0, col0); break;
            case 3: se_cov_tile<3, true>(xs, nt, nt, xs, nt, nt, se, diag_add, 1, 1, W, ld, 1, ec, row0, col0); break;
            default: se_cov_tile<0, true>(xs, nt, nt, xs, nt, nt, se, diag_add, 1, 1, W, ld, 1, ec, row0, col0); break;
            }
        }
}

// U = I (n x n, what small_potrf_partial<true> turns into L^-T): 16-byte stores (row pair of a thread; ld is even and the
// slice 16-byte aligned), then the diagonal
__device__ __forceinline__ void small_identity(double *U, int n, size_t ld, int tid)
{
    const int rp = 2 * (tid & 127), cp = tid >> 7;
    if (rp < n)
        for (int j = cp; j < n; j += 2) *reinterpret_cast<double2 *>(U + (size_t)rp + (size_t)j * ld) = make_double2(0.0, 0.0);
    __syncthreads();
    for (int i = tid; i < n; i += 256) U[(size_t)i * (ld + 1)] = 1.0;
}

// f_i = sum_{j <= i} W_ij z_j, columns 0 .. i IN ORDER with one accumulator (the order of k_trmv_lower_part within its
// first chunk: F is bit-identical between k_exact_gp_small, the VJP kernels and the blocked path), sixteen loads in
// flight per round trip -- a loop with one load per iteration is a chain of i memory latencies
__device__ __forceinline__ double small_tril_row_dot(const double *W, size_t ld, int i, const double *z)
{
    double acc = 0.0;
    for (int j0 = 0; j0 <= i; j0 += 16) {
        double u[16];
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int j = j0 + q <= i ? j0 + q : i;
            u[q] = W[(size_t)i + (size_t)j * ld];
        }
#pragma unroll
        for (int q = 0; q < 16; ++q)
            if (j0 + q <= i) acc = fma(u[q], z[j0 + q], acc);
    }
    return acc;
}

// sums of two 256-element LDS arrays into their elements 0: the tree of k_logml_partial (the same additions in the same
// order as the blocked path); the arrays are written and a barrier passed before the call, one is passed at the end
__device__ __forceinline__ void small_reduce2(double *s_a, double *s_b, int tid)
{
    for (int st = 128; st > 0; st >>= 1) {
        if (tid < st) {
            s_a[tid] += s_a[tid + st];
            s_b[tid] += s_b[tid + st];
        }
        __syncthreads();
    }
}

// lower triangle of the joint matrix [[K + s2 I, .], [Ks, Kss]] of the n points t and the m points ts, thread = row, and
// the augmented row [y^T, 0]; elem(blk, xi, xj): one covariance element of block blk = 0 (K), 1 (Ks), 2 (Kss)
template <class E>
__device__ __forceinline__ void small_joint_build(double *W, size_t ld, int n, int m, const double *t, const double *ts, const double *y,
                                                  double s2, int tid, E elem)
{
    const int nt = n + m;
    for (int i = tid; i < nt; i += 256) {
        const bool star = i >= n;
        const double xi = star ? ts[i - n] : t[i];
        const int jn = i < n ? i + 1 : n;
        for (int j = 0; j < jn; ++j) {
            double v = elem(star ? 1 : 0, xi, t[j]);
            if (i == j) v += s2;
            W[(size_t)i + (size_t)j * ld] = v;
        }
        for (int j = n; j <= i; ++j) W[(size_t)i + (size_t)j * ld] = elem(2, xi, ts[j - n]);
    }
    for (int j = tid; j < nt; j += 256) W[(size_t)nt + (size_t)j * ld] = j < n ? y[j] : 0.0;
}

// z = L11^-1 r for ONE right-hand row (W[row, 0 .. nb), stride ld) against the packed factors of a <= 128-order
// block in LDS: per 16-pivot block, z_kb = Linv16[kb] r_kb by 16 threads, then every row below subtracts
// L[r][kb] z_kb -- -L tiles and inverses in the fragment order potrf_diag4_body packs them in.
__device__ __forceinline__ void small_row_solve(const double *__restrict__ s_F, double *__restrict__ s_r,
                                                double *__restrict__ s_z, double *__restrict__ Wrow, size_t ld, int nb, int t)
{
    const int nblk = (nb + 15) >> 4;
    if (t < 128) s_r[t] = (t < nb) ? Wrow[(size_t)t * ld] : 0.0;
    __syncthreads();
    // every LDS read of a step is issued before its first use (fully unrolled, two accumulators): a loop with a
    // per-lane trip count made each of the 16 products wait for its own pair of reads (3 k cycles per step)
    for (int kb = 0; kb < nblk; ++kb) {
        if (t < 16) {
            double f[16], r[16];
#pragma unroll
            for (int c = 0; c < 16; ++c) {
                f[c] = s_F[fp_inv(kb) * 256 + (c >> 2) * 64 + (c & 3) * 16 + t];  // Linv16[t][c], zero above the diagonal
                r[c] = s_r[kb * 16 + c];
            }
            double z0 = 0.0, z1 = 0.0;
#pragma unroll
            for (int c = 0; c < 16; c += 2) {
                z0 = fma(f[c], r[c], z0);
                z1 = fma(f[c + 1], r[c + 1], z1);
            }
            s_z[kb * 16 + t] = z0 + z1;
        }
        __syncthreads();
        if (t < 128 && t >= (kb + 1) * 16 && t < nblk * 16) {
            const int jb = t >> 4, lr = t & 15;
            double f[16], z[16];
#pragma unroll
            for (int c = 0; c < 16; ++c) {
                f[c] = s_F[fp_l(jb, kb) * 256 + (c >> 2) * 64 + (c & 3) * 16 + lr];  // -L[t][16 kb + c]
                z[c] = s_z[kb * 16 + c];
            }
            double a0 = s_r[t], a1 = 0.0;
#pragma unroll
            for (int c = 0; c < 16; c += 2) {
                a0 = fma(f[c], z[c], a0);
                a1 = fma(f[c + 1], z[c + 1], a1);
            }
            s_r[t] = a0 + a1;
        }
        __syncthreads();
    }
    if (t < nb) Wrow[(size_t)t * ld] = s_z[t];
}

// Right-looking partial factorisation by ONE workgroup: the first nfac columns of the M x ncol lower trapezoid in
// W are factored, rows below / the trailing block updated (launch_potrf_partial's contract).  one_row: the caller
// promises M == ncol + 1 == nfac + 1 (one augmented row), which lets the last panel use small_row_solve.
// WITH_U (value + gradient kernels): U (same leading dimension, holds the identity on entry) becomes L^-T, block column
// by block column while that panel's packed factors are in LDS: column block k of U holds I - sum_{j < k} U[:, j] L[k, j]^T
// in its rows [0, k + nb) when panel k has been factored; the panel's strips apply L_kk^-T, and the panel's rows below
// (solved next) take the block out of the later column blocks in one product each.
template <bool WITH_U = false>
__device__ __forceinline__ void small_potrf_partial(double (&smem)[2][2][GK][GP], double *__restrict__ s_F,
                                                    double *__restrict__ s_aux, double *__restrict__ W, size_t ld, int M,
                                                    int ncol, int nfac, int *info, bool one_row, double *__restrict__ U = nullptr)
{
    const size_t ld0 = ld;
    // thread index, re-read behind an optimisation barrier in front of every phase: everything a phase derives from it
    // (LDS addresses, lane masks, column offsets: hundreds of values) is then computed where it is used instead of
    // being hoisted in front of the panel loop and kept in scratch memory across all phases
    auto fresh_tid = []() {
        int t = (int)threadIdx.x;
        asm volatile("" : "+v"(t));
        return t;
    };
    for (int k = 0; k < nfac; k += GPMI_NB) {
        const int nb = (nfac - k < GPMI_NB) ? nfac - k : GPMI_NB;
        // the leading dimension is made opaque per panel: otherwise every per-element offset of every phase (hundreds of
        // 64-bit values) is hoisted out of this loop and stays live across all phases -- the kernel then needs 512
        // registers, copies values through AGPRs around factor16's hand-scheduled DPP chain and breaks its hazard
        // assumptions (the hazard recogniser cannot see into the asm statements)
        size_t ld = ld0;
        asm volatile("" : "+s"(ld));
        double *Akk = W + (size_t)k + (size_t)k * ld;
        GPMI_STAMP(ts0)
        if (nb == GPMI_NB) potrf_diag4_body<false, true>(&smem[0][0][0][0], Akk, ld, nb, s_F, info, k, 8, fresh_tid());
        else potrf_diag4_body<false, false>(&smem[0][0][0][0], Akk, ld, nb, s_F, info, k, (nb + 15) >> 4, fresh_tid());
        __syncthreads();
        GPMI_STAMP(ts1)
        GPMI_STAMP_ADD(1, ts1 - ts0)
        if constexpr (WITH_U) {
            for (int rb = 0; rb < k + nb; rb += 64) {
                const int tid = fresh_tid();
                const int r = rb + (tid >> 6) * 16 + (tid & 15);
                // rows inside this panel are rows of the identity: zero left of their own 16-column block
                const int rw = rb + (tid >> 6) * 16 - k;
                const int kb0 = __builtin_amdgcn_readfirstlane(rw > 0 ? rw >> 4 : 0);
                if (nb == GPMI_NB && rb + 64 <= k + nb) trsm_panel_body<true>(s_F, U + (size_t)k * ld, ld, r, true, nb, tid, kb0);
                else trsm_panel_body<false>(s_F, U + (size_t)k * ld, ld, r, r < k + nb, nb, tid, kb0);
            }
            __syncthreads();
        }
        const int r0 = k + nb;
        if (r0 >= M) break;
        if (one_row && M - r0 == 1) {
            small_row_solve(s_F, s_aux, s_aux + 128, W + (size_t)r0 + (size_t)k * ld, ld, nb, fresh_tid());
            __syncthreads();
            GPMI_STAMP(ts2)
            GPMI_STAMP_ADD(2, ts2 - ts1)
            break;
        }
        // rows [r0, M): 16-row strips, one per wave, 64 rows per round
        for (int rb = r0; rb < M; rb += 64) {
            const int tid = fresh_tid();
            const int r = rb + (tid >> 6) * 16 + (tid & 15);
            if (nb == GPMI_NB && rb + 64 <= M) trsm_panel_body<true>(s_F, W + (size_t)k * ld, ld, r, true, nb, tid);
            else trsm_panel_body<false>(s_F, W + (size_t)k * ld, ld, r, r < M, nb, tid);
        }
        __syncthreads();
        GPMI_STAMP(ts2)
        GPMI_STAMP_ADD(2, ts2 - ts1)
        // trailing block: C[r0.., r0..ncol) -= X X^T, lower tiles
        const int mt = M - r0, nt = ncol - r0;
        if constexpr (WITH_U) {
            if (nt > 0) {  // U[0 : r0, r0 : ncol) -= U[0 : r0, k : r0) L[r0 : ncol, k : r0)^T
                for (int ti = 0; ti * GT < r0; ++ti)
                    for (int tj = 0; tj * GT < nt; ++tj) {
                        gemm_tile<0>(smem, U + (size_t)k * ld, ld, W + (size_t)r0 + (size_t)k * ld, ld, U + (size_t)r0 * ld, ld, r0, nt,
                                     nb, ti, tj, 0, fresh_tid());
                        __syncthreads();
                    }
            }
        }
        if (nt <= 0) continue;
        const double *X = W + (size_t)r0 + (size_t)k * ld;
        double *C = W + (size_t)r0 + (size_t)r0 * ld;
        const int T = (mt + GT - 1) / GT, TN = (nt + GT - 1) / GT;
        for (int ti = 0; ti < T; ++ti) {
            const int vr = (mt - ti * GT < GT) ? mt - ti * GT : GT;  // valid rows of this tile row
            if (vr == 1) {
                // ONE row below the square part (the augmented row y^T when the order is a multiple of 128): its update is
                // nt dot products of length nb -- thread = column, the row's panel entries from LDS, eight loads in flight --
                // instead of a 64 x 64 MFMA quadrant per 64 columns (8 k cycles each for one useful row)
                const int tid = fresh_tid(), row = ti * GT;
                __syncthreads();
                if (tid < nb) s_aux[tid] = X[(size_t)row + (size_t)tid * ld];
                __syncthreads();
                for (int j = tid; j < nt && j <= row; j += 256) {
                    double a0 = 0.0, a1 = 0.0;
                    for (int k0 = 0; k0 < nb; k0 += 8) {
                        double u[8];
#pragma unroll
                        for (int q = 0; q < 8; ++q) u[q] = X[(size_t)j + (size_t)(k0 + q < nb ? k0 + q : nb - 1) * ld];
#pragma unroll
                        for (int q = 0; q < 8; q += 2) {
                            a0 = fma(u[q], (k0 + q < nb) ? s_aux[k0 + q] : 0.0, a0);
                            a1 = fma(u[q + 1], (k0 + q + 1 < nb) ? s_aux[k0 + q + 1] : 0.0, a1);
                        }
                    }
                    C[(size_t)row + (size_t)j * ld] -= a0 + a1;
                }
                __syncthreads();
                continue;
            }
            for (int tj = 0; tj <= ti && tj < TN; ++tj) {
                if (vr <= 64 && nb % GK == 0) {  // thin tile row (e.g. the augmented row alone): 64-row quadrants
                    for (int qn = 0; qn < 2; ++qn) {
                        const int m0 = ti * GT, n0 = tj * GT + qn * 64;
                        if (n0 >= nt || (ti == tj && qn > 0)) continue;
                        gemm_quad64(&smem[0][0][0][0], X + m0, ld, X + n0, ld, C + (size_t)m0 + (size_t)n0 * ld, ld, nb, mt - m0,
                                    nt - n0, fresh_tid());
                        __syncthreads();
                    }
                } else {
                    gemm_tile<1>(smem, X, ld, X, ld, C, ld, mt, nt, nb, ti, tj, 0, fresh_tid());
                    __syncthreads();
                }
            }
        }
        GPMI_STAMP(ts3)
        GPMI_STAMP_ADD(4, ts3 - ts2)
    }
}

// One evaluation of models/fit_hyperparameters.stan:18-32 at n <= SMALL_N_MAX by one workgroup.
__device__ __forceinline__ void logml_small_body(double (&smem)[2][2][GK][GP], double *__restrict__ s_F, double *__restrict__ s_aux,
                                                 const double *__restrict__ X, int n, int ldx, const double *__restrict__ y,
                                                 const SmallSe &se, double diag_add, double *__restrict__ W, size_t ld,
                                                 double *__restrict__ out3, int *info_out, int *info_w, const ExpC &ec)
{
    const int tid = threadIdx.x;
    GPMI_STAMP(tb0)
    if (tid == 0) *info_w = 0;
    // covariance, lower 64 x 64 tiles, from the scaled coordinates staged ONCE in LDS (the staging buffer of the later
    // phases is free): one global round trip instead of one per tile and operand; y^T as row n
    {
        double *xs = &smem[0][0][0][0];
        small_scale_x(xs, X, n, ldx, se, tid);
        __syncthreads();
        small_se_build(xs, n, se, diag_add, W, ld, ec);
    }
    for (int j = tid; j < n; j += 256) W[(size_t)n + (size_t)j * ld] = y[j];
    __syncthreads();
    GPMI_STAMP(tb1)
    GPMI_STAMP_ADD(0, tb1 - tb0)
    GPMI_STAMP_ADD(3, 1)
    small_potrf_partial(smem, s_F, s_aux, W, ld, n + 1, n, n, info_w, true);
    GPMI_STAMP(tb2)
    // sum log L_ii, z'z: the reduction tree of k_logml_partial (slices of 256, thread `slice` keeps its sum) and, for more
    // than one slice, of k_logml_finalize over the slice sums -- the same additions in the same order as the blocked path
    double *s_a = s_aux, *s_b = s_aux + 256;
    const int nslice = (n + FIN_SLICE - 1) / FIN_SLICE;
    double pa = 0.0, pb = 0.0;
    for (int sl = 0; sl < nslice; ++sl) {
        const int i = sl * FIN_SLICE + tid;
        double a = 0.0, b = 0.0;
        if (i < n) {
            a = log(W[(size_t)i * (ld + 1)]);
            const double z = W[(size_t)n + (size_t)i * ld];
            b = z * z;
        }
        s_a[tid] = a;
        s_b[tid] = b;
        __syncthreads();
        small_reduce2(s_a, s_b, tid);
        if (nslice > 1) {
            if (tid == sl) {
                pa = s_a[0];
                pb = s_b[0];
            }
            __syncthreads();
        }
    }
    if (nslice > 1) {
        s_a[tid] = pa;
        s_b[tid] = pb;
        __syncthreads();
        small_reduce2(s_a, s_b, tid);
    }
    if (tid == 0) {
        const int info = __hip_atomic_load(info_w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (info_out) *info_out = info;
        if (info) {
            out3[0] = out3[1] = out3[2] = __builtin_nan("");
        } else {
            out3[1] = s_a[0];
            out3[2] = s_b[0];
            out3[0] = -0.5 * s_b[0] - s_a[0] - 0.5 * (double)n * 1.8378770664093454835606594728112;  // log(2 pi)
        }
    }
    GPMI_STAMP(tb3)
    GPMI_STAMP_ADD(5, tb3 - tb2)
}

// Value AND gradient sums of models/fit_hyperparameters.stan:18-32 by ONE workgroup (n <= 256, D <= GPMI_MAXD): what one
// leapfrog step of NUTS asks for at the sizes the reference's fits run (R/tests.R:5 N = 21, pendulum_fit.R 79 .. 199), where
// the launch chain of gpmi_logml_grad (factorisation, identity, L^-T, K^-1, contraction: ~25 launches + 4 copies) costs 150 us.
// d logml / d theta = 1/2 tr((a a' - K^-1) dK/dtheta): U = L^-T rides along in the factorisation (small_potrf_partial<true>),
// a = U z, K^-1 = U U^T by gemm_tile<2> over the lower tiles (only the columns >= the tile row's first: U is upper
// triangular), and the contraction re-evaluates the kernel from the scaled coordinates in LDS, thread = row.
// res: [0..2] logml, sum log L_ii, z'z; [3 + s] the contraction sums in the layout of k_grad_partial (GRAD_NS = 10 slots:
// [0] sum c, [1 + d] sum c (x_id - x_jd)^2, [9] sum_i g_ii) -- the host turns them into the gradient as for the chain.
constexpr int SMALL_GRAD_NS = 2 + GPMI_MAXD, SMALL_GRAD_RES = 3 + SMALL_GRAD_NS;
__device__ __forceinline__ void logml_grad_small_body(double (&smem)[2][2][GK][GP], double *__restrict__ s_F, double *__restrict__ s_aux,
                                                      const double *__restrict__ X, int n, int ldx, const double *__restrict__ y,
                                                      const SmallSe &se, double diag_add, double *__restrict__ W, size_t ld,
                                                      double *__restrict__ U, double *__restrict__ res, int *info_out, int *info_w,
                                                      const ExpC &ec)
{
    const int tid = threadIdx.x;
    GPMI_STAMP(tg0)
    if (tid == 0) *info_w = 0;
    double *xs = &smem[0][0][0][0];
    small_scale_x(xs, X, n, ldx, se, tid);
    __syncthreads();
    small_se_build(xs, n, se, diag_add, W, ld, ec);
    for (int j = tid; j < n; j += 256) W[(size_t)n + (size_t)j * ld] = y[j];
    small_identity(U, n, ld, tid);
    __syncthreads();
    GPMI_STAMP(tg1)
    GPMI_STAMP_ADD(0, tg1 - tg0)
    GPMI_STAMP_ADD(3, 1)
    small_potrf_partial<true>(smem, s_F, s_aux, W, ld, n + 1, n, n, info_w, true, U);
    __syncthreads();
    GPMI_STAMP(tg2)
    // value: one slice (n <= 256), the tree of k_logml_partial
    double *s_a = s_aux, *s_b = s_aux + 256, *s_z = s_aux + 512, *s_av = s_aux + 768;
    {
        double a = 0.0, b = 0.0, z = 0.0;
        if (tid < n) {
            a = log(W[(size_t)tid * (ld + 1)]);
            z = W[(size_t)n + (size_t)tid * ld];
            b = z * z;
        }
        s_a[tid] = a;
        s_b[tid] = b;
        s_z[tid] = z;
        __syncthreads();
        small_reduce2(s_a, s_b, tid);
    }
    const double sum_log = s_a[0], zz = s_b[0];
    // a = U z = K^-1 y (U upper triangular: the columns left of a wave's first row are zero); sixteen loads in flight per
    // round trip -- a loop with one load per iteration is a chain of n memory latencies
    {
        double acc0 = 0.0, acc1 = 0.0;
        const int ir = tid < n ? tid : n - 1;
        for (int j0 = tid & ~63; j0 < n; j0 += 16) {
            double u[16];
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int j = j0 + q < n ? j0 + q : n - 1;
                u[q] = U[(size_t)ir + (size_t)j * ld];
            }
#pragma unroll
            for (int q = 0; q < 16; q += 2) {
                acc0 = fma(u[q], (j0 + q < n) ? s_z[j0 + q] : 0.0, acc0);
                acc1 = fma(u[q + 1], (j0 + q + 1 < n) ? s_z[j0 + q + 1] : 0.0, acc1);
            }
        }
        s_av[tid] = acc0 + acc1;
    }
    // scaled coordinates for the contraction: in the packed-factor buffer (free now; the staging buffer is the product's)
    double *xg = s_F;
    small_scale_x(xg, X, n, ldx, se, tid);
    __syncthreads();
    GPMI_STAMP(tg3)
    GPMI_STAMP_ADD(5, tg3 - tg2)
    // K^-1 = U U^T tile by tile (lower tiles; only the columns >= the tile row's first), contracted where it is produced:
    // every element (m, n <= m) of a tile goes from its accumulator register into the sums -- K^-1 is never stored
    double acc[SMALL_GRAD_NS];
#pragma unroll
    for (int q = 0; q < SMALL_GRAD_NS; ++q) acc[q] = 0.0;
    const double a2 = se.a2;
    auto kinv_tiles = [&](auto dt) {
        constexpr int DT = decltype(dt)::value;   // compile-time dimension count (0: se.D at run time, <= GPMI_MAXD)
        const int Dn = DT ? DT : se.D;
        constexpr int DH = DT ? DT : 1;        // coordinates kept in registers per row / column (run-time D: re-read from LDS)
        double xm[4][DH], am[4], xn[DH], an = 0.0;
        int mm[4], ncur = 0;
        bool okn = false;
        auto contract = make_epi3(
            [&](int tm, int m, bool ok) {
                mm[tm] = ok ? m : -1;           // a row outside the matrix lies above every column: weight 0
                const int mc = ok ? m : 0;
                am[tm] = s_av[mc];
                if constexpr (DT != 0) {
#pragma unroll
                    for (int d = 0; d < DT; ++d) xm[tm][d] = xg[mc + d * n];
                }
            },
            [&](int nn, bool ok) {
                ncur = ok ? nn : 0;
                okn = ok;
                an = s_av[ncur];
                if constexpr (DT != 0) {
#pragma unroll
                    for (int d = 0; d < DT; ++d) xn[d] = xg[ncur + d * n];
                }
            },
            [&](double kinv, int tm) {
                double e = 0.0, r2[GPMI_MAXD];
                const int mc = mm[tm] < 0 ? 0 : mm[tm];
#pragma unroll
                for (int d = 0; d < (DT ? DT : GPMI_MAXD); ++d) {
                    double r;
                    if constexpr (DT != 0) r = xm[tm][d] - xn[d];
                    else r = d < Dn ? xg[mc + d * n] - xg[ncur + d * n] : 0.0;
                    r2[d] = r * r;
                    e += r2[d];
                }
                const double kse = a2 * exp_nonpos(-0.5 * e, ec);
                const double g = 0.5 * (am[tm] * an - kinv);
                const bool lower = okn && ncur <= mm[tm];
                const double c = lower ? ((ncur == mm[tm]) ? 1.0 : 2.0) * g * kse : 0.0;
                acc[0] += c;
#pragma unroll
                for (int d = 0; d < (DT ? DT : GPMI_MAXD); ++d) acc[1 + d] += c * r2[d];
                acc[1 + GPMI_MAXD] += (lower && ncur == mm[tm]) ? g : 0.0;
            });
        for (int ti = 0; ti * GT < n; ++ti)
            for (int tj = 0; tj <= ti; ++tj) {
                const int k0 = ti * GT;
                gemm_tile<3>(smem, U + (size_t)k0 * ld, ld, U + (size_t)k0 * ld, ld, W, ld, n, n, n - k0, ti, tj, 0, (int)threadIdx.x,
                             contract);
                __syncthreads();
            }
    };
    switch (se.D) {
    case 1: kinv_tiles(ic<1>{}); break;
    case 2: kinv_tiles(ic<2>{}); break;
    case 3: kinv_tiles(ic<3>{}); break;
    default: kinv_tiles(ic<0>{}); break;
    }
    GPMI_STAMP(tg4)
    GPMI_STAMP_ADD(6, tg4 - tg3)
#pragma unroll
    for (int d = 0; d < GPMI_MAXD; ++d)   // the sums are over UNSCALED squared differences (layout of k_grad_partial)
        acc[1 + d] = (d < se.D) ? acc[1 + d] / (se.inv_ell[d] * se.inv_ell[d]) : 0.0;
    __syncthreads();
    const int info = __hip_atomic_load(info_w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    // fixed-shape reduction (deterministic): butterfly inside every wave, the four wave sums added in wave order
#pragma unroll
    for (int q = 0; q < SMALL_GRAD_NS; ++q) {
        double v = acc[q];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
        if ((tid & 63) == 0) s_a[(tid >> 6) * SMALL_GRAD_NS + q] = v;
    }
    __syncthreads();
    if (tid < SMALL_GRAD_NS) {
        const double v = ((s_a[tid] + s_a[SMALL_GRAD_NS + tid]) + s_a[2 * SMALL_GRAD_NS + tid]) + s_a[3 * SMALL_GRAD_NS + tid];
        res[3 + tid] = info ? __builtin_nan("") : v;
    }
    GPMI_STAMP(tg5)
    GPMI_STAMP_ADD(7, tg5 - tg4)
    if (tid == 0) {
        if (info_out) *info_out = info;
        if (info) {
            res[0] = res[1] = res[2] = __builtin_nan("");
        } else {
            res[1] = sum_log;
            res[2] = zz;
            res[0] = -0.5 * zz - sum_log - 0.5 * (double)n * 1.8378770664093454835606594728112;  // log(2 pi)
        }
    }
}

// Completion flag of the one-launch host-buffer calls: the results lie in pinned, device-mapped host memory; every thread
// makes its stores visible system-wide, the workgroup meets, and thread 0 publishes `seq` -- the host polls the flag instead of
// paying a stream synchronisation (~8 us of a 30 us call).  done == nullptr: no flag.
__device__ __forceinline__ void small_signal_done(int *done, int seq)
{
    if (!done) return;   // kernel argument: workgroup-uniform
    __threadfence_system();
    __syncthreads();
    if (threadIdx.x == 0) __hip_atomic_store(done, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

constexpr int SMALL_PTS = 128;  // grid points per launch: their hyper-parameters travel as kernel arguments
struct SmallBatch {
    double a2[SMALL_PTS], inv_rho[SMALL_PTS], diag[SMALL_PTS];
};

// Workgroup memory of the small kernels: staging buffer of gemm_tile / workspace of the diagonal-block body, the
// packed factors of the current panel, reduction / substitution scratch.  DYNAMIC: with 148 KB of static LDS the
// compiler knows that one workgroup fits per CU, hands the kernel all 512 registers and moves values through AGPRs
// around factor16's hand-scheduled DPP chain -- whose hazard spacing (the recogniser cannot see into asm statements)
// it thereby breaks (v_accvgpr_read directly in front of a DPP read of the same register: wrong numbers).  With
// the size unknown at compile time __launch_bounds__(256, 2) holds and the kernel is allocated like k_gemm_nt<0>:
// <= 256 registers, no AGPR traffic.
constexpr int SMALL_LDS_DOUBLES = 2 * 2 * GK * GP + GPMI_FPACK + 512;
extern __shared__ __attribute__((aligned(16))) double small_lds[];
#define GPMI_SMALL_LDS                                                                                   \
    double (&smem)[2][2][GK][GP] = *reinterpret_cast<double (*)[2][2][GK][GP]>(small_lds);               \
    double *s_F = small_lds + 2 * 2 * GK * GP;                                                           \
    double *s_aux = s_F + GPMI_FPACK;

// stage (nullable): X and y are host-mapped memory (the host-buffer entry point): they are first copied, one
// coalesced pass with every load in flight (one PCIe round trip), to `stage` in device memory; out3 / info_out
// may likewise be host-mapped -- nothing is copied around the launch
__global__ __launch_bounds__(256, 2) void k_logml_small(const double *__restrict__ X, int n, int ldx, const double *__restrict__ y,
                                                     SeParams p, double diag_add, double *__restrict__ W, size_t ld,
                                                     double *__restrict__ out3, int *info_out, int *info_w, ExpC ec,
                                                     double *__restrict__ stage, int *done, int seq)
{
    GPMI_SMALL_LDS
    if (stage) {
        const int nx = n * p.D;
        small_stage(stage, n, threadIdx.x, X, p.D, ldx, y, 1, n);
        X = stage;
        y = stage + nx;
        ldx = n;
    }
    const SmallSe se = small_se(p.a2, p.inv_ell, p.D);
    logml_small_body(smem, s_F, s_aux, X, n, ldx, y, se, diag_add, W, ld, out3, info_out, info_w, ec);
    small_signal_done(done, seq);
}

// workgroup g = point g of the batch: isotropic (alpha, rho, sigma) as in gpmi_logml_grid; workspace slice g
__global__ __launch_bounds__(256, 2) void k_logml_small_batch(const double *__restrict__ X, int n, int ldx, int D,
                                                           const double *__restrict__ y, SmallBatch b, double *__restrict__ Wall,
                                                           size_t wstride, size_t ld, double *__restrict__ out3, int *info_out,
                                                           int *info_w, ExpC ec)
{
    GPMI_SMALL_LDS
    const int g = blockIdx.x;
    const SmallSe se = small_se_iso(b.a2[g], b.inv_rho[g], D);
    logml_small_body(smem, s_F, s_aux, X, n, ldx, y, se, b.diag[g], Wall + (size_t)g * wstride, ld, out3 + 3 * (size_t)g,
                     info_out + g, info_w + g, ec);
}

// the same with one length-scale PER DIMENSION and point (ARD grids: QQard takes a vector phi[[2]], R/kernels.R:11-19);
// 32 points per launch (their D <= 8 inverse length-scales travel as kernel arguments too)
constexpr int SMALL_PTS_ARD = 32;
struct SmallBatchArd {
    double a2[SMALL_PTS_ARD], diag[SMALL_PTS_ARD], inv_ell[SMALL_PTS_ARD][GPMI_MAXD];
};
__global__ __launch_bounds__(256, 2) void k_logml_small_batch_ard(const double *__restrict__ X, int n, int ldx, int D,
                                                               const double *__restrict__ y, SmallBatchArd b,
                                                               double *__restrict__ Wall, size_t wstride, size_t ld,
                                                               double *__restrict__ out3, int *info_out, int *info_w, ExpC ec)
{
    GPMI_SMALL_LDS
    const int g = blockIdx.x;
    const SmallSe se = small_se(b.a2[g], b.inv_ell[g], D);
    logml_small_body(smem, s_F, s_aux, X, n, ldx, y, se, b.diag[g], Wall + (size_t)g * wstride, ld, out3 + 3 * (size_t)g,
                     info_out + g, info_w + g, ec);
}

// Points whose hyper-parameters lie in DEVICE memory -- any number per launch, isotropic or ARD: par[g] = {alpha^2,
// sigma^2 + jitter, 1 / ell_0 .. 1 / ell_7}.  Used for grids of more than GPMI_SMALL_PTS points and for the mid sizes
// (n <= 1024) at which a grid large enough to give every CU a problem of its own beats the four lanes of the blocked path.
constexpr int SMALL_PAR = 2 + GPMI_MAXD;
__global__ __launch_bounds__(256, 2) void k_logml_small_batch_dev(const double *__restrict__ X, int n, int ldx, int D,
                                                               const double *__restrict__ y, const double *__restrict__ par,
                                                               double *__restrict__ Wall, size_t wstride, size_t ld,
                                                               double *__restrict__ out3, int *info_out, int *info_w, ExpC ec)
{
    GPMI_SMALL_LDS
    const int g = blockIdx.x;
    const double *pg = par + (size_t)g * SMALL_PAR;
    const SmallSe se = small_se(pg[0], pg + 2, D);
    logml_small_body(smem, s_F, s_aux, X, n, ldx, y, se, pg[1], Wall + (size_t)g * wstride, ld, out3 + 3 * (size_t)g,
                     info_out + g, info_w + g, ec);
}

// value + gradient sums: one evaluation (host-mapped X, y staged as in k_logml_small) ...
constexpr int SMALL_GRAD_LDS_DOUBLES = SMALL_LDS_DOUBLES + 512;   // s_aux: two reduction arrays + z + a
__global__ __launch_bounds__(256, 2) void k_logml_grad_small(const double *__restrict__ X, int n, int ldx, const double *__restrict__ y,
                                                          SeParams p, double diag_add, double *__restrict__ W, size_t ld,
                                                          double *__restrict__ U, double *__restrict__ res, int *info_out, int *info_w,
                                                          ExpC ec, double *__restrict__ stage, int *done, int seq)
{
    GPMI_SMALL_LDS
    if (stage) {
        const int nx = n * p.D;
        small_stage(stage, n, threadIdx.x, X, p.D, ldx, y, 1, n);
        X = stage;
        y = stage + nx;
        ldx = n;
    }
    const SmallSe se = small_se(p.a2, p.inv_ell, p.D);
    logml_grad_small_body(smem, s_F, s_aux, X, n, ldx, y, se, diag_add, W, ld, U, res, info_out, info_w, ec);
    small_signal_done(done, seq);
}

// ... and G isotropic points (the chains of a sampler: rstan's default is four), one workgroup each; slice g of Wall holds
// W and, ustride doubles behind it, U
__global__ __launch_bounds__(256, 2) void k_logml_grad_small_batch(const double *__restrict__ X, int n, int ldx, int D,
                                                                const double *__restrict__ y, SmallBatch b,
                                                                double *__restrict__ Wall, size_t wstride, size_t ustride, size_t ld,
                                                                double *__restrict__ res, int *info_out, int *info_w, ExpC ec,
                                                                double *__restrict__ stage, int *done, int seq, int *arrive)
{
    GPMI_SMALL_LDS
    const int g = blockIdx.x;
    if (stage) {   // X, y host-mapped (few chains: every workgroup stages its own copy, one PCIe round trip, side by side)
        double *st = stage + (size_t)g * n * (D + 1);
        const int nx = n * D;
        small_stage(st, n, threadIdx.x, X, D, ldx, y, 1, n);
        X = st;
        y = st + nx;
        ldx = n;
    }
    const SmallSe se = small_se_iso(b.a2[g], b.inv_rho[g], D);
    double *W = Wall + (size_t)g * wstride;
    logml_grad_small_body(smem, s_F, s_aux, X, n, ldx, y, se, b.diag[g], W, ld, W + ustride, res + (size_t)g * SMALL_GRAD_RES,
                          info_out + g, info_w + g, ec);
    if (done) {   // the LAST workgroup to finish publishes the completion flag (device counter `arrive`, re-armed by it)
        __threadfence_system();
        __syncthreads();
        if (threadIdx.x == 0) {
            const int k = __hip_atomic_fetch_add(arrive, 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
            if (k == (int)gridDim.x - 1) {
                __hip_atomic_store(arrive, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(done, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
            }
        }
    }
}

// ... and any number of points with one length-scale PER DIMENSION each, their SMALL_PAR records in device memory as for
// k_logml_small_batch_dev: the ARD grids of gpmi_logml_grad_grid_ard[_dev].  Device data only: no staging, no completion flag
__global__ __launch_bounds__(256, 2) void k_logml_grad_batch_dev(const double *__restrict__ X, int n, int ldx, int D,
                                                              const double *__restrict__ y, const double *__restrict__ par,
                                                              double *__restrict__ Wall, size_t wstride, size_t ustride, size_t ld,
                                                              double *__restrict__ res, int *info_out, int *info_w, ExpC ec)
{
    GPMI_SMALL_LDS
    const int g = blockIdx.x;
    const double *pg = par + (size_t)g * SMALL_PAR;
    const SmallSe se = small_se(pg[0], pg + 2, D);
    double *W = Wall + (size_t)g * wstride;
    logml_grad_small_body(smem, s_F, s_aux, X, n, ldx, y, se, pg[1], W, ld, W + ustride, res + (size_t)g * SMALL_GRAD_RES,
                          info_out + g, info_w + g, ec);
}

// One posterior draw of the derivative process (sample_derivs, pendulum_fit.R:227-255) per workgroup: the loop
// mclapply(s_list[1:100], sample_derivs_both_states, mc.cores = 2) (:261-268) is B independent draws, each with its own
// (l, a, sy) and noisy series, at n = m = 199 -- a chain of ~25 latency-bound launches per draw on the blocked path.  Here
// draw b builds [[a^2 QQ + sy^2 I, .], [a^2 RQ, a^2 RR]] with the row [y^T, 0] (the arithmetic of k_deriv_cov: deriv_val),
// factors the first n columns (Schur complement = cov - jitter I in the trailing block, -mu^T in the last row), adds the
// jitter, factors the m x m block in place and forms mu + chol(cov) z -- the composition of sample_derivs_core.
// par[3 g ..] = (l, a, sy) of draw g, in device memory (any number of draws per launch).
// status: 0, k (K + sy^2 I not PD at order k), n + k (cov).
__global__ __launch_bounds__(256, 2) void k_sample_derivs_small_batch(const double *__restrict__ t, int n, const double *__restrict__ ts,
                                                                   int m, const double *__restrict__ Y, const double *__restrict__ par,
                                                                   double jitter, const double *__restrict__ Z, double *__restrict__ Wall,
                                                                   size_t wstride, size_t ld, double *__restrict__ draws,
                                                                   double *__restrict__ mus, int *__restrict__ status,
                                                                   int *__restrict__ info_w)
{
    GPMI_SMALL_LDS
    const int g = blockIdx.x, tid = threadIdx.x;
    const int nt = n + m;
    double *W = Wall + (size_t)g * wstride;
    const double a2 = par[3 * g + 1] * par[3 * g + 1], l2 = par[3 * g] * par[3 * g], s2 = par[3 * g + 2] * par[3 * g + 2];
    const double *y = Y + (size_t)g * n, *z = Z + (size_t)g * m;
    int *iw = info_w + 2 * g;
    if (tid < 2) iw[tid] = 0;
    small_joint_build(W, ld, n, m, t, ts, y, s2, tid, [&](int blk, double xi, double xj) {
        return a2 * deriv_val(blk == 2 ? GPMI_RR : (blk ? GPMI_RQ : GPMI_QQ), xi, xj, l2);
    });
    __syncthreads();
    small_potrf_partial(smem, s_F, s_aux, W, ld, nt + 1, nt, n, iw, false);
    __syncthreads();
    double *S = W + (size_t)n + (size_t)n * ld;
    for (int j = tid; j < m; j += 256) {
        S[(size_t)j * (ld + 1)] += jitter;
        const double mu = -W[(size_t)nt + (size_t)(n + j) * ld];
        mus[(size_t)g * m + j] = mu;
    }
    __syncthreads();
    small_potrf_partial(smem, s_F, s_aux, S, ld, m, m, m, iw + 1, false);
    __syncthreads();
    // draw = mu + L z: row i, columns 0 .. i in order (the order of k_trmv_lower_part within a chunk), sixteen loads in flight
    // (not small_tril_row_dot: rows past 256 take further rounds, and the column bound is workgroup-uniform here)
    for (int i0 = 0; i0 < m; i0 += 256) {
        const int i = i0 + tid, ic = i < m ? i : m - 1;
        double acc = 0.0;
        const int jend = (i0 + 255 < m ? i0 + 255 : m - 1);   // workgroup-uniform bound; columns > i contribute exact zeros
        for (int j0 = 0; j0 <= jend; j0 += 16) {
            double u[16];
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int j = j0 + q <= ic ? j0 + q : ic;
                u[q] = S[(size_t)ic + (size_t)j * ld];
            }
#pragma unroll
            for (int q = 0; q < 16; ++q)
                if (j0 + q <= ic) acc = fma(u[q], z[j0 + q], acc);
        }
        if (i < m) draws[(size_t)g * m + i] = acc + mus[(size_t)g * m + i];
    }
    __syncthreads();
    if (tid == 0) {
        const int i1 = __hip_atomic_load(iw, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const int i2 = __hip_atomic_load(iw + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        status[g] = i1 ? i1 : (i2 ? n + i2 : 0);
    }
}

// gpmi_gp_condition (p_Xn / p_dotXn, R/ode_gp.R:1-32; the moments of sample_derivs) at the sizes R/tests.R runs it by ONE
// workgroup: joint matrix [[K + s2 I, .], [Ks, Kss]] with the row [y^T, 0] (deriv_cov_val: the arithmetic of k_deriv_cov),
// partial factorisation of the first n columns, then Kn = Schur complement mirrored + jitter I and mn = minus the last row --
// the launch chain's nine kernels and six copies in one launch.  stage (nullable): t, ts, y are host-mapped and are copied
// to device memory first; Kn / mn / info_out may be host-mapped as well.
struct CondArgs {
    int kindK, kindS, kindSS, compat;
    double a2, l2, s2, jitter;
};
__global__ __launch_bounds__(256, 2) void k_gp_condition_small(const double *__restrict__ t, int n, const double *__restrict__ ts, int m,
                                                            const double *__restrict__ y, CondArgs q, double *__restrict__ W, size_t ld,
                                                            double *__restrict__ Kn, size_t ldo, double *__restrict__ mn, int *info_out,
                                                            int *info_w, double *__restrict__ stage, int *done, int seq)
{
    GPMI_SMALL_LDS
    const int tid = threadIdx.x, nt = n + m;
    if (stage) {
        for (int e = tid; e < 2 * n + m; e += 256) stage[e] = e < n ? t[e] : (e < nt ? ts[e - n] : y[e - nt]);
        __syncthreads();
        t = stage;
        ts = stage + n;
        y = stage + nt;
    }
    if (tid == 0) *info_w = 0;
    small_joint_build(W, ld, n, m, t, ts, y, q.s2, tid, [&](int blk, double xi, double xj) {
        return deriv_cov_val(blk == 2 ? q.kindSS : (blk ? q.kindS : q.kindK), q.compat, q.a2, xi, xj, q.l2);
    });
    __syncthreads();
    small_potrf_partial(smem, s_F, s_aux, W, ld, nt + 1, nt, n, info_w, false);
    __syncthreads();
    const double *S = W + (size_t)n + (size_t)n * ld;
    for (int r = tid; r < m; r += 256) {
        for (int c = 0; c < m; ++c) {
            double v = (r >= c) ? S[(size_t)r + (size_t)c * ld] : S[(size_t)c + (size_t)r * ld];
            if (r == c) v += q.jitter;
            Kn[(size_t)r + (size_t)c * ldo] = v;
        }
        mn[r] = -W[(size_t)nt + (size_t)(n + r) * ld];
    }
    if (tid == 0) *info_out = __hip_atomic_load(info_w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    small_signal_done(done, seq);
}

// gpmi_gp_predict (pointwise posterior mean and variance at m new D-dimensional inputs; what the sweep of R/tests.R:89-97 asks
// of create_p_dotXnS, R/ode_gp_library.R:43-93) at the reference's sizes by ONE workgroup: joint matrix
// [[K + diag_add I, .], [Ks, alpha^2 on the diagonal]] of the n + m points [X; Xs] built with se_cov_tile (the arithmetic of
// gpmi_se_cov), the row [y^T, 0], partial factorisation of the first n columns; the Schur block's diagonal is then var and the
// last row -mean.  X, Xs, y are read exactly once each (into LDS / the workspace), so host-mapped inputs need no staging copy;
// mean / var (nullable) / info_out may be host-mapped as well.
__global__ __launch_bounds__(256, 2) void k_gp_predict_small(const double *__restrict__ X, int n, int ldx, const double *__restrict__ Xs,
                                                          int m, int ldxs, const double *__restrict__ y, SeParams p, double diag_add,
                                                          double *__restrict__ W, size_t ld, double *__restrict__ mean,
                                                          double *__restrict__ var, int *info_out, int *info_w, ExpC ec, int *done,
                                                          int seq)
{
    GPMI_SMALL_LDS
    int tid = threadIdx.x;
    const int nt = n + m;
    if (tid == 0) *info_w = 0;
    const SmallSe se = small_se(p.a2, p.inv_ell, p.D);
    {
        double *xs = &smem[0][0][0][0];   // nt * D <= 1024 * GPMI_MAXD doubles fit the tile staging buffer
        // (not small_scale_x: the n + m points come from two arrays, X and Xs, in one pass)
#pragma unroll
        for (int d = 0; d < GPMI_MAXD; ++d)
            if (d < se.D)
                for (int i = tid; i < nt; i += 256)
                    xs[i + d * nt] = __dmul_rn(i < n ? X[(size_t)i + (size_t)d * ldx] : Xs[(size_t)(i - n) + (size_t)d * ldxs], se.inv_ell[d]);
        __syncthreads();
        small_se_build(xs, nt, se, diag_add, W, ld, ec);
    }
    __syncthreads();
    // the new points carry the latent function's prior variance: no noise term on their diagonal
    for (int i = n + tid; i < nt; i += 256) W[(size_t)i * (ld + 1)] = se.a2;
    for (int j = tid; j < nt; j += 256) W[(size_t)nt + (size_t)j * ld] = j < n ? y[j] : 0.0;
    __syncthreads();
    small_potrf_partial(smem, s_F, s_aux, W, ld, nt + 1, nt, n, info_w, false);
    __syncthreads();
    // (as in the VJP body: what the read-out derives from the thread index is formed here, not kept live, i.e. spilled, across the
    // factorisation: 80 B of scratch per lane with it, 88 without)
    asm volatile("" : "+v"(tid));
    const int info = __hip_atomic_load(info_w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    for (int r = tid; r < m; r += 256) {
        const size_t c = (size_t)(n + r);
        mean[r] = info ? __builtin_nan("") : -W[(size_t)nt + c * ld];
        if (var) var[r] = info ? __builtin_nan("") : W[c * (ld + 1)];
    }
    if (tid == 0) *info_out = info;
    small_signal_done(done, seq);
}

// gpmi_gp_predict_joint (the JOINT posterior at m new D-dimensional inputs: mean, covariance and draws; what create_p_dotXnS,
// R/ode_gp_library.R:43-93, conditions on, without its sequential loop) by ONE workgroup: the build and the first partial
// factorisation of k_gp_predict_small; then mean = minus the last row and cov = the mirrored Schur block + post_jitter I
// (k_gp_condition_small's read-out); then, for B > 0 columns, the second factorisation in place and draws[:, b] = mean + Lc Z[:, b]
// by the row loop of k_sample_derivs_small_batch, column b of Z staged in LDS (read once: Z may be host-mapped like every
// other pointer but W and info_w).  A row's sum runs over its columns in order with one accumulator, whatever B is.
// status: 0, k (Sigma not PD at order k: every output NaN), n + k (cov not PD: draws NaN, mean and cov as with B = 0).
__global__ __launch_bounds__(256, 2) void k_gp_predict_joint_wg(const double *__restrict__ X, int n, int ldx, const double *__restrict__ Xs,
                                                             int m, int ldxs, const double *__restrict__ y, SeParams p, double diag_add,
                                                             double post_jitter, double *__restrict__ W, size_t ld,
                                                             double *__restrict__ mean, double *__restrict__ cov, size_t ldc,
                                                             const double *__restrict__ Z, int B, size_t ldz,
                                                             double *__restrict__ draws, size_t ldd, int *info_out, int *info_w, ExpC ec,
                                                             int *done, int seq)
{
    GPMI_SMALL_LDS
    int tid = threadIdx.x;
    const int nt = n + m;
    if (tid < 2) info_w[tid] = 0;
    const SmallSe se = small_se(p.a2, p.inv_ell, p.D);
    {
        double *xs = &smem[0][0][0][0];   // nt * D <= 1024 * GPMI_MAXD doubles fit the tile staging buffer
#pragma unroll
        for (int d = 0; d < GPMI_MAXD; ++d)
            if (d < se.D)
                for (int i = tid; i < nt; i += 256)
                    xs[i + d * nt] = __dmul_rn(i < n ? X[(size_t)i + (size_t)d * ldx] : Xs[(size_t)(i - n) + (size_t)d * ldxs], se.inv_ell[d]);
        __syncthreads();
        small_se_build(xs, nt, se, diag_add, W, ld, ec);
    }
    __syncthreads();
    for (int i = n + tid; i < nt; i += 256) W[(size_t)i * (ld + 1)] = se.a2;
    for (int j = tid; j < nt; j += 256) W[(size_t)nt + (size_t)j * ld] = j < n ? y[j] : 0.0;
    __syncthreads();
    small_potrf_partial(smem, s_F, s_aux, W, ld, nt + 1, nt, n, info_w, false);
    __syncthreads();
    asm volatile("" : "+v"(tid));
    const int info = __hip_atomic_load(info_w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    double *S = W + (size_t)n + (size_t)n * ld;   // Schur complement (lower), rows n .. nt - 1
    // thread = row: its own diagonal element takes post_jitter (for the read-out and for the factorisation below); nothing else
    // of the block is written here, so no thread reads what another one changes
    for (int r = tid; r < m; r += 256) {
        mean[r] = info ? __builtin_nan("") : -W[(size_t)nt + (size_t)(n + r) * ld];
        S[(size_t)r * (ld + 1)] += post_jitter;
        if (cov)
            for (int c = 0; c < m; ++c) {
                const double v = (r >= c) ? S[(size_t)r + (size_t)c * ld] : S[(size_t)c + (size_t)r * ld];
                cov[(size_t)r + (size_t)c * ldc] = info ? __builtin_nan("") : v;
            }
    }
    int info2 = 0;
    if (B > 0) {   // kernel argument: workgroup-uniform
        __syncthreads();
        if (!info) {
            small_potrf_partial(smem, s_F, s_aux, S, ld, m, m, m, info_w + 1, false);
            __syncthreads();
            asm volatile("" : "+v"(tid));
            info2 = __hip_atomic_load(info_w + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        const bool bad = info || info2;
        double *zl = &smem[0][0][0][0];   // m <= 1023 doubles
        for (int b = 0; b < B; ++b) {
            for (int j = tid; j < m; j += 256) zl[j] = Z[(size_t)j + (size_t)b * ldz];
            __syncthreads();
            for (int i0 = 0; i0 < m; i0 += 256) {
                const int i = i0 + tid, ic = i < m ? i : m - 1;
                double acc = 0.0;
                const int jend = (i0 + 255 < m ? i0 + 255 : m - 1);   // workgroup-uniform bound; columns > i contribute nothing
                for (int j0 = 0; j0 <= jend; j0 += 16) {
                    double u[16];
#pragma unroll
                    for (int q = 0; q < 16; ++q) {
                        const int j = j0 + q <= ic ? j0 + q : ic;
                        u[q] = S[(size_t)ic + (size_t)j * ld];
                    }
#pragma unroll
                    for (int q = 0; q < 16; ++q)
                        if (j0 + q <= ic) acc = fma(u[q], zl[j0 + q], acc);
                }
                if (i < m) draws[(size_t)i + (size_t)b * ldd] = bad ? __builtin_nan("") : acc - W[(size_t)nt + (size_t)(n + i) * ld];
            }
            __syncthreads();
        }
    }
    if (tid == 0) *info_out = info ? info : (info2 ? n + info2 : 0);
    small_signal_done(done, seq);
}

// gpmi_joint_predict (the posterior of f, f', f'' at m new times given stacked observations yy = [y; y'] under the joint model
// of R/ode_gp_library.R:29-30; pendulum_fit3.R:31-46 observes both series) by ONE workgroup, the composition of
// k_gp_predict_joint_wg with the matrices of the joint model.  thread = POINT for the build: a training point i writes its
// entries of S with the arithmetic of k_joint_cov (the bits of gpmi_joint_logml's matrix), a new point its rows of the p star
// blocks (deriv_val_pair: the bits of k_deriv_cov) from one exponential per pair of points; t and ts are staged in LDS (read
// once: every pointer but W and info_w may be host-mapped).  Then the partial factorisation of the first 2n columns, mean =
// minus the last row, cov = the mirrored Schur block + pj[a] on block a, and for B > 0 the second factorisation and the row
// loop of the draws, exactly as in k_gp_predict_joint_wg.  Workspace rows: 2n of S, m per requested order, the row [yy^T, 0].
// status: 0, k (S not PD at order k: every output NaN), 2n + k (cov not PD: draws NaN, mean and cov as with B = 0).
struct JointPredArgs {
    double a2, l2, s2, jitter, pj0, pj1, pj2;   // pj*: post_jitter of the first, second, third REQUESTED order
    int orders;
};
__global__ __launch_bounds__(256, 2) void k_joint_predict_wg(const double *__restrict__ t, int n, const double *__restrict__ ts, int m,
                                                          const double *__restrict__ yy, JointPredArgs q, double *__restrict__ W,
                                                          size_t ld, double *__restrict__ mean, double *__restrict__ cov, size_t ldc,
                                                          const double *__restrict__ Z, int B, size_t ldz, double *__restrict__ draws,
                                                          size_t ldd, int *info_out, int *info_w, ExpC ec, int *done, int seq)
{
    GPMI_SMALL_LDS
    int tid = threadIdx.x;
    const int n2 = 2 * n, p = __builtin_popcount(q.orders), pm = p * m, nt = n2 + pm;
    if (tid < 2) info_w[tid] = 0;
    {
        double *xs = &smem[0][0][0][0];   // n + m <= 1023 doubles: t, then ts
        for (int i = tid; i < n + m; i += 256) xs[i] = i < n ? t[i] : ts[i - n];
        __syncthreads();
        const double il2 = 1.0 / q.l2;
        for (int i = tid; i < n + m; i += 256) {
            const double xi = xs[i];
            if (i < n) {   // rows i and n + i of S: QQ and RR lower, RQ in full (k_joint_cov with compat = 0)
                for (int j = 0; j < n; ++j) {
                    const double r0 = xi - xs[j];
                    const double e0 = exp_nonpos(-(r0 * r0 / (2 * q.l2)), ec);
                    W[(size_t)(n + i) + (size_t)j * ld] = -(q.a2 * e0 * r0 * il2);
                    if (j <= i) {
                        double qq = q.a2 * e0, rr = q.a2 * e0 * il2 - q.a2 * e0 * r0 * r0 * il2 * il2;
                        if (i == j) { qq += q.s2 + q.jitter; rr += q.jitter; }
                        W[(size_t)i + (size_t)j * ld] = qq;
                        W[(size_t)(n + i) + (size_t)(n + j) * ld] = rr;
                    }
                }
            } else {   // rows 2n + ia m + ii of the star blocks
                const int ii = i - n;
                const int jn = p > 1 ? n + m : i + 1;   // one order: its only block is lower-stored
                for (int j = 0; j < jn; ++j) {
                    const double yv = xs[j];
                    const double d = xi - yv, b = yv - xi;
                    const double e = exp(-(d * d / (2 * q.l2)));   // deriv_val's argument
                    int ia = 0;
                    for (int a = 0; a < 3; ++a) {
                        if (!((q.orders >> a) & 1)) continue;
                        double *Wr = W + (size_t)n2 + (size_t)ia * m + (size_t)ii;
                        if (j < n) {
                            Wr[(size_t)j * ld] = q.a2 * deriv_val_pair(a, 0, d, b, e, q.l2);
                            Wr[(size_t)(n + j) * ld] = q.a2 * deriv_val_pair(a, 1, d, b, e, q.l2);
                        } else {
                            int ib = 0;
                            for (int o = 0; o <= a; ++o) {
                                if (!((q.orders >> o) & 1)) continue;
                                if (o < a || j <= i) Wr[(size_t)(n2 + ib * m + j - n) * ld] = q.a2 * deriv_val_pair(a, o, d, b, e, q.l2);
                                ++ib;
                            }
                        }
                        ++ia;
                    }
                }
            }
        }
    }
    for (int j = tid; j < nt; j += 256) W[(size_t)nt + (size_t)j * ld] = j < n2 ? yy[j] : 0.0;
    __syncthreads();
    small_potrf_partial(smem, s_F, s_aux, W, ld, nt + 1, nt, n2, info_w, false);
    __syncthreads();
    asm volatile("" : "+v"(tid));
    const int info = __hip_atomic_load(info_w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    double *S = W + (size_t)n2 + (size_t)n2 * ld;   // Schur complement (lower), rows 2n .. nt - 1
    // thread = row: its own diagonal element takes its block's post_jitter (for the read-out and for the factorisation below);
    // nothing else of the block is written here, so no thread reads what another one changes
    for (int r = tid; r < pm; r += 256) {
        mean[r] = info ? __builtin_nan("") : -W[(size_t)nt + (size_t)(n2 + r) * ld];
        S[(size_t)r * (ld + 1)] += r < m ? q.pj0 : (r < 2 * m ? q.pj1 : q.pj2);
        if (cov)
            for (int c = 0; c < pm; ++c) {
                const double v = (r >= c) ? S[(size_t)r + (size_t)c * ld] : S[(size_t)c + (size_t)r * ld];
                cov[(size_t)r + (size_t)c * ldc] = info ? __builtin_nan("") : v;
            }
    }
    int info2 = 0;
    if (B > 0) {   // kernel argument: workgroup-uniform
        __syncthreads();
        if (!info) {
            small_potrf_partial(smem, s_F, s_aux, S, ld, pm, pm, pm, info_w + 1, false);
            __syncthreads();
            asm volatile("" : "+v"(tid));
            info2 = __hip_atomic_load(info_w + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        const bool bad = info || info2;
        double *zl = &smem[0][0][0][0];   // pm <= 1021 doubles
        for (int b = 0; b < B; ++b) {
            for (int j = tid; j < pm; j += 256) zl[j] = Z[(size_t)j + (size_t)b * ldz];
            __syncthreads();
            for (int i0 = 0; i0 < pm; i0 += 256) {
                const int i = i0 + tid, ic = i < pm ? i : pm - 1;
                double acc = 0.0;
                const int jend = (i0 + 255 < pm ? i0 + 255 : pm - 1);   // workgroup-uniform bound; columns > i contribute nothing
                for (int j0 = 0; j0 <= jend; j0 += 16) {
                    double u[16];
#pragma unroll
                    for (int k = 0; k < 16; ++k) {
                        const int j = j0 + k <= ic ? j0 + k : ic;
                        u[k] = S[(size_t)ic + (size_t)j * ld];
                    }
#pragma unroll
                    for (int k = 0; k < 16; ++k)
                        if (j0 + k <= ic) acc = fma(u[k], zl[j0 + k], acc);
                }
                if (i < pm) draws[(size_t)i + (size_t)b * ldd] = bad ? __builtin_nan("") : acc - W[(size_t)nt + (size_t)(n2 + i) * ld];
            }
            __syncthreads();
        }
    }
    if (tid == 0) *info_out = info ? info : (info2 ? n2 + info2 : 0);
    small_signal_done(done, seq);
}

// f = chol(cov_exp_quad(X, alpha, ell) + diag_add I) z (models/exact_gp.stan:17-25: the latent exact GP's transform, once per
// leapfrog step with a new length-scale) by ONE workgroup for n <= 256: build (se_cov_tile), factorisation, and the row sums
// f_i = sum_{j <= i} L_ij z_j in column order (the order of k_trmv_lower_part inside its first chunk).  stage (nullable): X, z
// host-mapped -> copied to device memory first; f / info_out may be host-mapped.
__global__ __launch_bounds__(256, 2) void k_exact_gp_small(const double *__restrict__ X, int n, int ldx, const double *__restrict__ z,
                                                        SeParams p, double diag_add, double *__restrict__ W, size_t ld,
                                                        double *__restrict__ f, int *info_out, int *info_w, ExpC ec,
                                                        double *__restrict__ stage, int *done, int seq)
{
    GPMI_SMALL_LDS
    const int tid = threadIdx.x;
    if (stage) {
        const int nx = n * p.D;
        small_stage(stage, n, tid, X, p.D, ldx, z, 1, n);
        X = stage;
        z = stage + nx;
        ldx = n;
    }
    if (tid == 0) *info_w = 0;
    const SmallSe se = small_se(p.a2, p.inv_ell, p.D);
    {
        double *xs = &smem[0][0][0][0];
        small_scale_x(xs, X, n, ldx, se, tid);
        __syncthreads();
        small_se_build(xs, n, se, diag_add, W, ld, ec);
    }
    __syncthreads();
    small_potrf_partial(smem, s_F, s_aux, W, ld, n, n, n, info_w, false);
    __syncthreads();
    if (tid < n) s_aux[tid] = z[tid];
    __syncthreads();
    if (tid < n) {
        const int i = tid;
        const double acc = small_tril_row_dot(W, ld, i, s_aux);
        const int info = __hip_atomic_load(info_w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        f[i] = info ? __builtin_nan("") : acc;
    }
    if (tid == 0) *info_out = __hip_atomic_load(info_w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    small_signal_done(done, seq);
}

// The vector-Jacobian product of the same transform for k <= GPMI_VJP_KMAX columns (F = L Z; adjoint Fbar), what NUTS asks of
// models/exact_gp.stan:17-25 (and, k = 2, of models/heteroscedastic.stan:23-32) at every leapfrog step, by ONE workgroup for
// n <= 256.  The chain of gpmi_api.hip (exact_gp_vjp_core) states the algebra; here:
//   build, factorisation with U = L^-T riding along (small_potrf_partial<true>, as k_logml_grad_small);
//   F column by column with the loop of k_exact_gp_small (bit-identical to the value call);
//   Zbar = W = L^T Fbar, thread = column of L;
//   V = U Phi(W Z^T) by the suffix sums along the rows of U o w_c, thread = row;
//   2 Sbar = V U^T + U V^T = [V U] [U V]^T by gemm_tile<3> with K = 2n (V, U, V stored side by side, so that ONE product per
//   tile forms it) and contracted in registers against dK/dtheta as logml_grad_small_body contracts K^-1.
// R: 3 n columns of leading dimension ld, [V | U | V]; the gradient (1 + n_ell) is finished on the device.
constexpr int VJP_KMAX = GPMI_VJP_KMAX;
// HEAD: Fbar is not an input but the adjoint of a likelihood head evaluated on F (gpmi_latent_gp_lp_grad): F is formed
// unconditionally, thread = row evaluates latent_head_row (k <= 2), lik and d lik / d sigma are reduced in a fixed order into
// out[0..1], and Fb (nullable) receives the Fbar the sweep then uses.  Everything else is the same statement for both instances.
template <bool HEAD>
__device__ __forceinline__ void exact_gp_vjp_small_body(const double *__restrict__ X, int n, int ldx, const SeParams &p,
                                                        double diag_add, const double *__restrict__ Z, int k, int ldz,
                                                        std::conditional_t<HEAD, double, const double> *__restrict__ Fb, int ldfb,
                                                        double *__restrict__ F, int ldf, double *__restrict__ Zb, int ldzb,
                                                        double *__restrict__ W, double *__restrict__ R, size_t ld, double alpha,
                                                        const GradEll &el, int n_ell, double *__restrict__ grad, int *info_out,
                                                        int *info_w, const ExpC &ec, double *__restrict__ stage, int *done, int seq,
                                                        const LatentHead &lh, double *__restrict__ out)
{
    GPMI_SMALL_LDS
    constexpr int KM = HEAD ? 2 : VJP_KMAX;   // columns the per-column loops unroll for (the heads have k <= 2)
    // HEAD: at its phase boundaries below the thread index passes through an empty asm, so that what later phases derive from it
    // (row and column addresses the compiler would otherwise form early) is not kept live, i.e. spilled, across the head's
    // exp / log1p: with these the instance needs the scratch of the plain one (3824 B per lane), without them 56 B more
    int tid = threadIdx.x;
    if (stage) {   // host-mapped X, Z, Fbar (HEAD: Y): one coalesced pass into device memory
        const int nx = n * p.D, nz = n * k;
        if constexpr (HEAD) {
            small_stage(stage, n, tid, X, p.D, ldx, Z, k, ldz, lh.Y, lh.m, lh.ldy);
        } else {
            small_stage(stage, n, tid, X, p.D, ldx, Z, k, ldz, Fb, k, ldfb);
            Fb = stage + nx + nz;
            ldfb = n;
        }
        X = stage;
        Z = stage + nx;
        ldx = ldz = n;
    }
    if (tid == 0) *info_w = 0;
    const SmallSe se = small_se(p.a2, p.inv_ell, p.D);
    double *V = R, *U = R + (size_t)n * ld, *V2 = R + 2 * (size_t)n * ld;
    {
        double *xs = &smem[0][0][0][0];
        small_scale_x(xs, X, n, ldx, se, tid);
        __syncthreads();
        small_se_build(xs, n, se, diag_add, W, ld, ec);
    }
    if constexpr (HEAD) asm volatile("" : "+v"(tid));   // (HEAD, as below: 3820 B of scratch per lane with this one, 3840 without)
    small_identity(U, n, ld, tid);
    __syncthreads();
    small_potrf_partial<true>(smem, s_F, s_aux, W, ld, n, n, n, info_w, false, U);
    __syncthreads();
    if constexpr (HEAD) asm volatile("" : "+v"(tid));
    const int info = __hip_atomic_load(info_w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    // the packed factors are no longer needed: s_F holds the scaled coordinates, Fbar (then W) and Z, k n doubles each
    double *xg = s_F, *s_w = s_F + 2048, *s_z = s_F + 4096;
    small_scale_x(xg, X, n, ldx, se, tid);
    for (int e = tid; e < n * k; e += 256) {
        const int c = e / n, i = e - c * n;
        s_z[e] = Z[(size_t)i + (size_t)c * ldz];
        if constexpr (!HEAD) s_w[e] = Fb[(size_t)i + (size_t)c * ldfb];
    }
    __syncthreads();
    // F, one column at a time: the loop of k_exact_gp_small (row sums in column order).  Written out, not small_tril_row_dot: the
    // same operations in the same order, but through the helper k_exact_gp_vjp_small needs 56 B more scratch per lane
    if constexpr (HEAD) asm volatile("" : "+v"(tid));
    if (HEAD || F)
        for (int c = 0; c < k; ++c) {
            if (tid < n) {
                const int i = tid;
                const double *zc = s_z + c * n;
                double acc = 0.0;
                for (int j0 = 0; j0 <= i; j0 += 16) {
                    double u[16];
#pragma unroll
                    for (int q = 0; q < 16; ++q) {
                        const int j = j0 + q <= i ? j0 + q : i;
                        u[q] = W[(size_t)i + (size_t)j * ld];
                    }
#pragma unroll
                    for (int q = 0; q < 16; ++q)
                        if (j0 + q <= i) acc = fma(u[q], zc[j0 + q], acc);
                }
                if (F) F[(size_t)i + (size_t)c * ldf] = info ? __builtin_nan("") : acc;
                if constexpr (HEAD) s_w[c * n + i] = acc;   // the head reads its row of F here and leaves Fbar
            }
        }
    if constexpr (HEAD) {
        // the head on this thread's row, Fbar into LDS where the sweep reads it; lik and d lik / d sigma by a butterfly inside
        // every wave and the four wave sums added in wave order
        double red0 = 0.0, red1 = 0.0, fb0 = 0.0, fb1 = 0.0;
        if (tid < n) {
            // Y: the copy made at entry when staged (derived here rather than kept live across the factorisation)
            const LatentHead hd{lh.family, stage ? stage + n * (p.D + k) : lh.Y, lh.m, stage ? n : lh.ldy, lh.sigma, lh.log_sigma};
            latent_head_row(hd, s_w[tid], k > 1 ? s_w[n + tid] : 0.0, hd.Y + tid, red0, red1, fb0, fb1);
            for (int c = 0; c < k; ++c) {
                const double v = c ? fb1 : fb0;
                s_w[c * n + tid] = v;
                if (Fb) Fb[(size_t)tid + (size_t)c * ldfb] = info ? __builtin_nan("") : v;
            }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            red0 += __shfl_xor(red0, off, 64);
            red1 += __shfl_xor(red1, off, 64);
        }
        if ((tid & 63) == 0) {
            s_aux[(tid >> 6) * 2] = red0;
            s_aux[(tid >> 6) * 2 + 1] = red1;
        }
        __syncthreads();   // (also: every row of Fbar is in s_w)
        if (tid < 2) out[tid] = info ? __builtin_nan("") : ((s_aux[tid] + s_aux[2 + tid]) + s_aux[4 + tid]) + s_aux[6 + tid];
        asm volatile("" : "+v"(tid));
    }
    // W = L^T Fbar: thread = column j of L, all k columns at once
    double wj[KM];
#pragma unroll
    for (int c = 0; c < KM; ++c) wj[c] = 0.0;
    if (tid < n) {
        const int j = tid;
        const double *col = W + (size_t)j * ld;
        for (int i0 = j; i0 < n; i0 += 8) {
            double l8[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) l8[q] = col[i0 + q < n ? i0 + q : n - 1];
#pragma unroll
            for (int q = 0; q < 8; ++q)
                if (i0 + q < n)
#pragma unroll
                    for (int c = 0; c < KM; ++c)
                        if (c < k) wj[c] = fma(l8[q], s_w[c * n + i0 + q], wj[c]);
        }
    }
    __syncthreads();   // every thread has read Fbar
    if (tid < n)
#pragma unroll
        for (int c = 0; c < KM; ++c)
            if (c < k) {
                s_w[c * n + tid] = wj[c];
                Zb[(size_t)tid + (size_t)c * ldzb] = info ? __builtin_nan("") : wj[c];
            }
    __syncthreads();
    if constexpr (HEAD) asm volatile("" : "+v"(tid));
    // V = U Phi(W Z^T): thread = row i, columns from the last to the first, one running suffix sum per column of Z
    if (tid < n) {
        const int i = tid;
        double P[KM];
#pragma unroll
        for (int c = 0; c < KM; ++c) P[c] = 0.0;
        for (int j1 = n; j1 > 0; j1 -= 16) {
            double u[16];
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int j = j1 - 1 - q;
                u[q] = (j >= i) ? U[(size_t)i + (size_t)j * ld] : 0.0;
            }
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int j = j1 - 1 - q;
                if (j < 0) break;
                double v = 0.0;
#pragma unroll
                for (int c = 0; c < KM; ++c)
                    if (c < k) {
                        const double t = u[q] * s_w[c * n + j];
                        v = fma(s_z[c * n + j], fma(0.5, t, P[c]), v);
                        P[c] += t;
                    }
                V[(size_t)i + (size_t)j * ld] = v;
                V2[(size_t)i + (size_t)j * ld] = v;
            }
        }
    }
    __syncthreads();
    if constexpr (HEAD) asm volatile("" : "+v"(tid));
    // [V U] [U V]^T tile by tile (lower tiles), contracted where it is produced; the columns of [V U] left of the tile's first
    // column are skipped (U's rows there are zero in V U^T; U V^T needs them all)
    double acc[1 + GPMI_MAXD];
#pragma unroll
    for (int q = 0; q < 1 + GPMI_MAXD; ++q) acc[q] = 0.0;
    const double a2 = se.a2;
    auto sbar_tiles = [&](auto dt) {
        constexpr int DT = decltype(dt)::value;   // compile-time dimension count (0: se.D at run time, <= GPMI_MAXD)
        const int Dn = DT ? DT : se.D;
        constexpr int DH = DT ? DT : 1;
        double xm[4][DH], xn[DH];
        int mm[4], ncur = 0;
        bool okn = false;
        auto contract = make_epi3(
            [&](int tm, int m, bool ok) {
                mm[tm] = ok ? m : -1;
                if constexpr (DT != 0) {
                    const int mc = ok ? m : 0;
#pragma unroll
                    for (int d = 0; d < DT; ++d) xm[tm][d] = xg[mc + d * n];
                }
            },
            [&](int nn, bool ok) {
                ncur = ok ? nn : 0;
                okn = ok;
                if constexpr (DT != 0) {
#pragma unroll
                    for (int d = 0; d < DT; ++d) xn[d] = xg[ncur + d * n];
                }
            },
            [&](double s2, int tm) {
                double e = 0.0, r2[GPMI_MAXD];
                const int mc = mm[tm] < 0 ? 0 : mm[tm];
#pragma unroll
                for (int d = 0; d < (DT ? DT : GPMI_MAXD); ++d) {
                    double r;
                    if constexpr (DT != 0) r = xm[tm][d] - xn[d];
                    else r = d < Dn ? xg[mc + d * n] - xg[ncur + d * n] : 0.0;
                    r2[d] = r * r;
                    e += r2[d];
                }
                const double kse = a2 * exp_nonpos(-0.5 * e, ec);
                const bool lower = okn && ncur <= mm[tm];
                const double c = lower ? ((ncur == mm[tm]) ? 0.5 : 1.0) * s2 * kse : 0.0;
                acc[0] += c;
#pragma unroll
                for (int d = 0; d < (DT ? DT : GPMI_MAXD); ++d) acc[1 + d] += c * r2[d];
            });
        for (int ti = 0; ti * GT < n; ++ti)
            for (int tj = 0; tj <= ti; ++tj) {
                const int k0 = tj * GT;
                gemm_tile<3>(smem, R + (size_t)k0 * ld, ld, U + (size_t)k0 * ld, ld, W, ld, n, n, 2 * n - k0, ti, tj, 0,
                             (int)threadIdx.x, contract);
                __syncthreads();
            }
    };
    switch (se.D) {
    case 1: sbar_tiles(ic<1>{}); break;
    case 2: sbar_tiles(ic<2>{}); break;
    case 3: sbar_tiles(ic<3>{}); break;
    default: sbar_tiles(ic<0>{}); break;
    }
#pragma unroll
    for (int d = 0; d < GPMI_MAXD; ++d)   // sums over UNSCALED squared differences (layout of k_grad_partial)
        acc[1 + d] = (d < se.D) ? acc[1 + d] / (se.inv_ell[d] * se.inv_ell[d]) : 0.0;
    // fixed-shape reduction: butterfly inside every wave, the four wave sums added in wave order
    double *s_r = s_aux;
#pragma unroll
    for (int q = 0; q < 1 + GPMI_MAXD; ++q) {
        double v = acc[q];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
        if ((tid & 63) == 0) s_r[(tid >> 6) * (1 + GPMI_MAXD) + q] = v;
    }
    __syncthreads();
    if (tid < 1 + GPMI_MAXD) {
        constexpr int S = 1 + GPMI_MAXD;
        s_r[4 * S + tid] = ((s_r[tid] + s_r[S + tid]) + s_r[2 * S + tid]) + s_r[3 * S + tid];
    }
    __syncthreads();
    if (tid == 0) {
        const double nan = __builtin_nan("");
        if (info)
            for (int q = 0; q <= n_ell; ++q) grad[q] = nan;
        else
            gpmi_grad_from_sums(s_r + 4 * (1 + GPMI_MAXD), se.D, alpha, el.ell, n_ell, grad);
        *info_out = info;
    }
    small_signal_done(done, seq);
}

__global__ __launch_bounds__(256, 2) void k_exact_gp_vjp_small(const double *__restrict__ X, int n, int ldx, SeParams p, double diag_add,
                                                            const double *__restrict__ Z, int k, int ldz, const double *__restrict__ Fb,
                                                            int ldfb, double *__restrict__ F, int ldf, double *__restrict__ Zb, int ldzb,
                                                            double *__restrict__ W, double *__restrict__ R, size_t ld, double alpha,
                                                            GradEll el, int n_ell, double *__restrict__ grad, int *info_out,
                                                            int *info_w, ExpC ec, double *__restrict__ stage, int *done, int seq)
{
    exact_gp_vjp_small_body<false>(X, n, ldx, p, diag_add, Z, k, ldz, Fb, ldfb, F, ldf, Zb, ldzb, W, R, ld, alpha, el, n_ell,
                                   grad, info_out, info_w, ec, stage, done, seq, LatentHead{}, nullptr);
}

// forward product, likelihood head, its adjoint and the reverse sweep in one launch (gpmi_latent_gp_lp_grad, n <= 256, k <= 2):
// out[0] = lik, out[1] = d lik / d sigma; Fb (nullable) receives Fbar
__global__ __launch_bounds__(256, 2) void k_latent_gp_small(const double *__restrict__ X, int n, int ldx, SeParams p, double diag_add,
                                                         const double *__restrict__ Z, int k, int ldz, LatentHead lh,
                                                         double *__restrict__ out, double *__restrict__ Fb, int ldfb,
                                                         double *__restrict__ F, int ldf, double *__restrict__ Zb, int ldzb,
                                                         double *__restrict__ W, double *__restrict__ R, size_t ld, double alpha,
                                                         GradEll el, int n_ell, double *__restrict__ grad, int *info_out, int *info_w,
                                                         ExpC ec, double *__restrict__ stage, int *done, int seq)
{
    exact_gp_vjp_small_body<true>(X, n, ldx, p, diag_add, Z, k, ldz, Fb, ldfb, F, ldf, Zb, ldzb, W, R, ld, alpha, el, n_ell, grad, info_out,
                                  info_w, ec, stage, done, seq, lh, out);
}

// The CENTRED latent GP (models/heteroscedastic_centered.stan:24-34; gpmi_centered_gp_lp_grad) by ONE workgroup for n <= 256,
// D <= GPMI_MAXD, k <= CEN_KMAX: the k latent columns are parameters with the GP as their prior.  logml_grad_small_body with k
// augmented rows instead of one:
//   build; F^T rides as rows n .. n + k - 1 of the partial factorisation and comes out as Z^T, U = L^-T rides along
//   (small_potrf_partial<true>); sum log L_ii and sum_c z_c'z_c by the tree of k_logml_partial;
//   a_c = U z_c for all columns in one pass over U (thread = row); the head on this thread's row of F, Fgrad = Fbar - a;
//   Sigma^-1 = U U^T tile by tile, contracted in registers with g_ij = 1/2 (sum_c a_ic a_jc - k Sigma^-1_ij) against dSigma/dtheta.
// W: n + k rows; out (4), Fg (n x k, ldfg), grad (1 + n_ell) and info_out may be host-mapped (stage != null: n (D + k + m)
// doubles of device scratch receive X, F and Y in one coalesced pass).  The gradient is finished on the device.
constexpr int CEN_KMAX = GPMI_CEN_KMAX;
__global__ __launch_bounds__(256, 2) void k_centered_gp_small(const double *__restrict__ X, int n, int ldx, SeParams p, double diag_add,
                                                           const double *__restrict__ F, int k, int ldf, LatentHead lh,
                                                           double *__restrict__ out, double *__restrict__ Fg, int ldfg,
                                                           double *__restrict__ W, double *__restrict__ U, size_t ld, double alpha,
                                                           GradEll el, int n_ell, double *__restrict__ grad, int *info_out,
                                                           int *info_w, ExpC ec, double *__restrict__ stage, int *done, int seq)
{
    GPMI_SMALL_LDS
    int tid = threadIdx.x;
    const bool head = lh.family != GPMI_LIK_NONE;
    if (stage) {   // host-mapped X, F, Y: one coalesced pass into device memory
        const int nx = n * p.D;
        small_stage(stage, n, tid, X, p.D, ldx, F, k, ldf, lh.Y, head ? lh.m : 0, lh.ldy);
        X = stage;
        F = stage + nx;
        ldx = ldf = n;
    }
    if (tid == 0) *info_w = 0;
    const SmallSe se = small_se(p.a2, p.inv_ell, p.D);
    {
        double *xs = &smem[0][0][0][0];
        small_scale_x(xs, X, n, ldx, se, tid);
        __syncthreads();
        small_se_build(xs, n, se, diag_add, W, ld, ec);
    }
    for (int c = 0; c < k; ++c)   // F^T as rows n .. n + k - 1
        for (int j = tid; j < n; j += 256) W[(size_t)(n + c) + (size_t)j * ld] = F[(size_t)j + (size_t)c * ldf];
    small_identity(U, n, ld, tid);
    __syncthreads();
    small_potrf_partial<true>(smem, s_F, s_aux, W, ld, n + k, n, n, info_w, k == 1, U);
    __syncthreads();
    asm volatile("" : "+v"(tid));
    const int info = __hip_atomic_load(info_w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    // the packed factors are no longer needed: s_F holds the scaled coordinates, A = Sigma^-1 F and Z, k n doubles each
    double *xg = s_F, *s_av = s_F + 2048, *s_z = s_F + 4096;
    double *s_a = s_aux, *s_b = s_aux + 256;
    small_scale_x(xg, X, n, ldx, se, tid);
    {   // value: one slice (n <= 256), the tree of k_logml_partial; the squares of a row's k entries of Z in column order
        double a = 0.0, b = 0.0;
        if (tid < n) {
            a = log(W[(size_t)tid * (ld + 1)]);
            for (int c = 0; c < k; ++c) {
                const double z = W[(size_t)(n + c) + (size_t)tid * ld];
                s_z[c * n + tid] = z;
                b += z * z;
            }
        }
        s_a[tid] = a;
        s_b[tid] = b;
        __syncthreads();
        small_reduce2(s_a, s_b, tid);
    }
    const double sum_log = s_a[0], zz = s_b[0];
    __syncthreads();   // (s_a, s_b are written again below)
    // A = U Z (U upper triangular: the columns left of a wave's first row are zero): one pass over U for all k columns,
    // sixteen loads in flight per round trip
    double av[CEN_KMAX];
#pragma unroll
    for (int c = 0; c < CEN_KMAX; ++c) av[c] = 0.0;
    {
        const int ir = tid < n ? tid : n - 1;
        for (int j0 = tid & ~63; j0 < n; j0 += 16) {
            double u[16];
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int j = j0 + q < n ? j0 + q : n - 1;
                u[q] = U[(size_t)ir + (size_t)j * ld];
            }
#pragma unroll
            for (int q = 0; q < 16; ++q)
                if (j0 + q < n)
#pragma unroll
                    for (int c = 0; c < CEN_KMAX; ++c)
                        if (c < k) av[c] = fma(u[q], s_z[c * n + j0 + q], av[c]);
        }
    }
    if (tid < n)
#pragma unroll
        for (int c = 0; c < CEN_KMAX; ++c)
            if (c < k) s_av[c * n + tid] = av[c];
    // the head on this thread's row of F; Fgrad = Fbar - A; lik and d lik / d sigma by a butterfly inside every wave and the
    // four wave sums added in wave order
    {
        double red0 = 0.0, red1 = 0.0, fb0 = 0.0, fb1 = 0.0;
        if (tid < n) {
            if (head) {
                const LatentHead hd{lh.family, stage ? stage + n * (p.D + k) : lh.Y, lh.m, stage ? n : lh.ldy, lh.sigma, lh.log_sigma};
                latent_head_row(hd, F[tid], k > 1 ? F[(size_t)tid + (size_t)ldf] : 0.0, hd.Y + tid, red0, red1, fb0, fb1);
            }
#pragma unroll
            for (int c = 0; c < CEN_KMAX; ++c)
                if (c < k) {
                    const double fb = c == 0 ? fb0 : (c == 1 ? fb1 : 0.0);
                    Fg[(size_t)tid + (size_t)c * ldfg] = info ? __builtin_nan("") : fb - av[c];
                }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            red0 += __shfl_xor(red0, off, 64);
            red1 += __shfl_xor(red1, off, 64);
        }
        if ((tid & 63) == 0) {
            s_b[(tid >> 6) * 2] = red0;
            s_b[(tid >> 6) * 2 + 1] = red1;
        }
    }
    __syncthreads();   // (also: every row of A is in s_av, the coordinates in xg)
    const double lik = ((s_b[0] + s_b[2]) + s_b[4]) + s_b[6], dsig = ((s_b[1] + s_b[3]) + s_b[5]) + s_b[7];
    asm volatile("" : "+v"(tid));
    // Sigma^-1 = U U^T tile by tile (lower tiles; only the columns >= the tile row's first), contracted where it is produced
    double acc[1 + GPMI_MAXD];
#pragma unroll
    for (int q = 0; q < 1 + GPMI_MAXD; ++q) acc[q] = 0.0;
    const double a2 = se.a2, kd = (double)k;
    auto kinv_tiles = [&](auto dt) {
        constexpr int DT = decltype(dt)::value;   // compile-time dimension count (0: se.D at run time, <= GPMI_MAXD)
        const int Dn = DT ? DT : se.D;
        constexpr int DH = DT ? DT : 1;
        double xm[4][DH], am[4], xn[DH], an = 0.0;
        int mm[4], ncur = 0;
        bool okn = false;
        auto contract = make_epi3(
            [&](int tm, int m, bool ok) {
                mm[tm] = ok ? m : -1;           // a row outside the matrix lies above every column: weight 0
                const int mc = ok ? m : 0;
                am[tm] = s_av[mc];
                if constexpr (DT != 0) {
#pragma unroll
                    for (int d = 0; d < DT; ++d) xm[tm][d] = xg[mc + d * n];
                }
            },
            [&](int nn, bool ok) {
                ncur = ok ? nn : 0;
                okn = ok;
                an = s_av[ncur];
                if constexpr (DT != 0) {
#pragma unroll
                    for (int d = 0; d < DT; ++d) xn[d] = xg[ncur + d * n];
                }
            },
            [&](double kinv, int tm) {
                double e = 0.0, r2[GPMI_MAXD];
                const int mc = mm[tm] < 0 ? 0 : mm[tm];
#pragma unroll
                for (int d = 0; d < (DT ? DT : GPMI_MAXD); ++d) {
                    double r;
                    if constexpr (DT != 0) r = xm[tm][d] - xn[d];
                    else r = d < Dn ? xg[mc + d * n] - xg[ncur + d * n] : 0.0;
                    r2[d] = r * r;
                    e += r2[d];
                }
                const double kse = a2 * exp_nonpos(-0.5 * e, ec);
                double aa = am[tm] * an;        // sum_c a_mc a_nc, columns in index order (the first pair from registers)
                for (int c = 1; c < k; ++c) aa += s_av[c * n + mc] * s_av[c * n + ncur];
                const double g = 0.5 * (aa - kd * kinv);
                const bool lower = okn && ncur <= mm[tm];
                const double cc = lower ? ((ncur == mm[tm]) ? 1.0 : 2.0) * g * kse : 0.0;
                acc[0] += cc;
#pragma unroll
                for (int d = 0; d < (DT ? DT : GPMI_MAXD); ++d) acc[1 + d] += cc * r2[d];
            });
        for (int ti = 0; ti * GT < n; ++ti)
            for (int tj = 0; tj <= ti; ++tj) {
                const int k0 = ti * GT;
                gemm_tile<3>(smem, U + (size_t)k0 * ld, ld, U + (size_t)k0 * ld, ld, W, ld, n, n, n - k0, ti, tj, 0, (int)threadIdx.x,
                             contract);
                __syncthreads();
            }
    };
    switch (se.D) {
    case 1: kinv_tiles(ic<1>{}); break;
    case 2: kinv_tiles(ic<2>{}); break;
    case 3: kinv_tiles(ic<3>{}); break;
    default: kinv_tiles(ic<0>{}); break;
    }
#pragma unroll
    for (int d = 0; d < GPMI_MAXD; ++d)   // sums over UNSCALED squared differences (layout of k_grad_partial)
        acc[1 + d] = (d < se.D) ? acc[1 + d] / (se.inv_ell[d] * se.inv_ell[d]) : 0.0;
    // fixed-shape reduction: butterfly inside every wave, the four wave sums added in wave order
    double *s_r = s_aux;
#pragma unroll
    for (int q = 0; q < 1 + GPMI_MAXD; ++q) {
        double v = acc[q];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
        if ((tid & 63) == 0) s_r[(tid >> 6) * (1 + GPMI_MAXD) + q] = v;
    }
    __syncthreads();
    if (tid < 1 + GPMI_MAXD) {
        constexpr int S = 1 + GPMI_MAXD;
        s_r[4 * S + tid] = ((s_r[tid] + s_r[S + tid]) + s_r[2 * S + tid]) + s_r[3 * S + tid];
    }
    __syncthreads();
    if (tid == 0) {
        const double nan = __builtin_nan("");
        if (info)
            for (int q = 0; q <= n_ell; ++q) grad[q] = nan;
        else
            gpmi_grad_from_sums(s_r + 4 * (1 + GPMI_MAXD), se.D, alpha, el.ell, n_ell, grad);
        out[0] = info ? nan : (-0.5 * zz - kd * sum_log) + lik;
        out[1] = info ? nan : dsig;
        out[2] = info ? nan : sum_log;
        out[3] = info ? nan : zz;
        *info_out = info;
    }
    small_signal_done(done, seq);
}

// rbf_cov_chol (covariance.cpp:9-47) by ONE workgroup for n <= 128 (test_interpolate.R:5 runs it at N = 100, P = 10 times):
// Sigma_ij = exp(-(x_i - x_j)^2 / (2 l^2)) + 1e-10 [i == j], L = chol(Sigma), and the forward-mode tangent
// dL/dl = L Phi(L^-1 Sdot L^-T), Sdot_ij = Sigma_ij (x_i - x_j)^2 / l^3, Phi = lower triangle with halved diagonal --
// the launch chain of rbf_cov_chol_core (build, factor, copy, tangent build, two panel solves, two transposes, mask, product:
// ~12 launches) with the same device functions back to back.  Workgroup g handles length-scale ls[g] and writes L (upper
// zeroed) and dL/dl (lower; its upper triangle exact zeros) to Lout + g ostride, dLout + g ostride (leading dimension ldo;
// device or host-mapped memory).  Workspace per workgroup: three slices of small_ws_layout(n) (Sigma / L, S, S2).
struct RbfBatch {
    double l[64];
};
__global__ __launch_bounds__(256, 2) void k_rbf_cov_chol_small(const double *__restrict__ x, int n, RbfBatch ls, double *__restrict__ Wall,
                                                            size_t wstride, size_t ld, double *__restrict__ Lout,
                                                            double *__restrict__ dLout, size_t ostride, size_t ldo, int *info_out,
                                                            int *info_w, ExpC ec, double *__restrict__ stage)
{
    GPMI_SMALL_LDS
    const int g = blockIdx.x, tid = threadIdx.x;
    const double l = ls.l[g];
    double *W = Wall + (size_t)g * 3 * wstride, *S = W + wstride, *S2 = S + wstride;
    double *Lo = Lout + (size_t)g * ostride, *dLo = dLout + (size_t)g * ostride;
    int *iw = info_w + g;
    if (stage) {   // x host-mapped: one copy per workgroup
        double *st = stage + (size_t)g * n;
        for (int i = tid; i < n; i += 256) st[i] = x[i];
        __syncthreads();
        x = st;
    }
    if (tid == 0) *iw = 0;
    const SmallSe se = small_se_iso(1.0, 1.0 / l, 1);
    double *xs = &smem[0][0][0][0];
    small_scale_x(xs, x, n, n, se, tid);
    __syncthreads();
    small_se_build(xs, n, se, 1e-10, W, ld, ec);
    // Sdot, full (the arithmetic of k_rbf_dsigma), thread = row
    for (int i = tid; i < n; i += 256) {
        const double xi = x[i];
        for (int j = 0; j < n; ++j) {
            const double r = xi - x[j], r2 = r * r;
            S[(size_t)i + (size_t)j * ld] = exp(-r2 / (2 * l * l)) * r2 / (l * l * l);
        }
    }
    __syncthreads();
    const int nblk = (n + 15) >> 4;
    if (n == GPMI_NB) potrf_diag4_body<false, true>(&smem[0][0][0][0], W, ld, n, s_F, iw, 0, 8, tid);
    else potrf_diag4_body<false, false>(&smem[0][0][0][0], W, ld, n, s_F, iw, 0, nblk, tid);
    __syncthreads();
    // (the element-wise passes below keep eight loads in flight per round trip: a loop with one dependent load per iteration
    // is a chain of n memory latencies -- 100 us per pass at n = 100)
    // L out, and its upper triangle zeroed in place: W is the A operand of the last product
    for (int i = tid; i < n; i += 256)
        for (int j0 = 0; j0 < n; j0 += 8) {
            double v[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const int j = j0 + q < n ? j0 + q : n - 1;
                v[q] = W[(size_t)i + (size_t)j * ld];
            }
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const int j = j0 + q;
                if (j < n) {
                    if (j > i) W[(size_t)i + (size_t)j * ld] = 0.0;
                    Lo[(size_t)i + (size_t)j * ldo] = (j <= i) ? v[q] : 0.0;
                }
            }
        }
    auto solve_rows = [&](double *A) {   // A <- A L^-T, all n rows, 64 per round
        for (int rb = 0; rb < n; rb += 64) {
            const int r = rb + (tid >> 6) * 16 + (tid & 15);
            if (n == GPMI_NB && rb + 64 <= n) trsm_panel_body<true>(s_F, A, ld, r, true, n, tid);
            else trsm_panel_body<false>(s_F, A, ld, r, r < n, n, tid);
        }
        __syncthreads();
    };
    solve_rows(S);                                                  // S = Sdot L^-T
    for (int i = tid; i < n; i += 256)                              // S2 = S^T = L^-1 Sdot
        for (int j0 = 0; j0 < n; j0 += 8) {
            double v[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) v[q] = S[(size_t)(j0 + q < n ? j0 + q : n - 1) + (size_t)i * ld];
#pragma unroll
            for (int q = 0; q < 8; ++q)
                if (j0 + q < n) S2[(size_t)i + (size_t)(j0 + q) * ld] = v[q];
        }
    __syncthreads();
    solve_rows(S2);                                                 // S2 = M = L^-1 Sdot L^-T
    // B operand of the product: row j, column k holds Phi(M)[k][j]  (k >= j; the diagonal halved)
    for (int j = tid; j < n; j += 256)
        for (int k0 = 0; k0 < n; k0 += 8) {
            double v[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) v[q] = S2[(size_t)(k0 + q < n ? k0 + q : n - 1) + (size_t)j * ld];
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const int k = k0 + q;
                if (k < n) S[(size_t)j + (size_t)k * ld] = (k > j) ? v[q] : ((k == j) ? 0.5 * v[q] : 0.0);
            }
        }
    __syncthreads();
    gemm_tile<2>(smem, W, ld, S, ld, dLo, ldo, n, n, n, 0, 0, 0, tid);   // dL = L Phi (n <= 128: one tile)
    __syncthreads();
    if (tid == 0) info_out[g] = __hip_atomic_load(iw, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// stream-ordered upload of up to PUT_MAX doubles that travel as kernel arguments (no staging buffer whose reuse would
// have to be fenced against an earlier asynchronous call)
constexpr int PUT_MAX = 480;
struct PutArgs {
    double v[PUT_MAX];
};
__global__ __launch_bounds__(256) void k_put_doubles(PutArgs a, double *__restrict__ dst, int count)
{
    for (int i = threadIdx.x; i < count; i += 256) dst[i] = a.v[i];
}

// the factorisation alone (launch_potrf_partial at small sizes: posteriors, rbf_cov_chol, ...)
__global__ __launch_bounds__(256, 2) void k_potrf_small(double *__restrict__ W, size_t ld, int M, int ncol, int nfac, int *info)
{
    GPMI_SMALL_LDS
    small_potrf_partial(smem, s_F, s_aux, W, ld, M, ncol, nfac, info, false);
}
#undef GPMI_SMALL_LDS

}  // namespace

// ---------------------------------------------------------------------------
// host-side drivers
// ---------------------------------------------------------------------------
// Every small kernel is launched with 256 threads and more dynamic workgroup memory than the default limit (see
// SMALL_LDS_DOUBLES): the limit of THAT kernel is raised once per device (the flags are per instantiation, i.e. per kernel)
template <auto Kernel, class... Args>
static void launch_small(int grid, int lds_doubles, hipStream_t s, Args... args)
{
    static bool done[64];
    int dev = 0;
    if (hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < 64 && !done[dev]) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  lds_doubles * (int)sizeof(double));
        done[dev] = true;
    }
    hipLaunchKernelGGL(Kernel, dim3(grid), 256, lds_doubles * sizeof(double), s, args...);
}

// G isotropic points (alpha, rho, sigma) as kernel arguments
static SmallBatch small_batch(const double *alpha, const double *rho, const double *sigma, int G, double jitter)
{
    SmallBatch b;
    for (int g = 0; g < G; ++g) {
        b.a2[g] = alpha[g] * alpha[g];
        b.inv_rho[g] = 1.0 / rho[g];
        b.diag[g] = sigma[g] * sigma[g] + jitter;
    }
    return b;
}

// ---- small-N evaluations: one workgroup each ------------------------------------------------
// workspace slice of one n-point problem: leading dimension and stride (doubles) between consecutive slices
void small_ws_layout(int n, size_t *ld, size_t *stride)
{
    *ld = (size_t)(((n + 1 + 15) / 16) * 16 + 16);
    *stride = *ld * (size_t)(n + 1) + 256;  // tile loads may over-read rows past the end of the last column
}

void launch_logml_small(hipStream_t s, const double *dX, int n, int ldx, const double *dy, const SeParams &p, double diag_add,
                        double *W, size_t ld, double *d_out3, int *d_info_out, int *d_info_work, double *stage, int *done, int seq)
{
    launch_small<k_logml_small>(1, SMALL_LDS_DOUBLES, s, dX, n, ldx, dy, p, diag_add, W, ld, d_out3,
                       d_info_out, d_info_work, h_exp, stage, done, seq);
}

// G <= GPMI_SMALL_PTS points (alpha, rho, sigma) in ONE launch of G workgroups; Wall: G slices (small_ws_layout)
void launch_logml_small_batch(hipStream_t s, const double *dX, int n, int ldx, int D, const double *dy, const double *alpha,
                              const double *rho, const double *sigma, int G, double jitter, double *Wall, double *d_out3,
                              int *d_info_out, int *d_info_work)
{
    static_assert(SMALL_PTS == GPMI_SMALL_PTS, "batch size of the small-N grid launch");
    const SmallBatch b = small_batch(alpha, rho, sigma, G, jitter);
    size_t ld, stride;
    small_ws_layout(n, &ld, &stride);
    launch_small<k_logml_small_batch>(G, SMALL_LDS_DOUBLES, s, dX, n, ldx, D, dy, b, Wall, stride, ld, d_out3, d_info_out,
                       d_info_work, h_exp);
}

// G <= GPMI_SMALL_PTS_ARD points with a length-scale per dimension: ell is G x D, point-major
void launch_logml_small_batch_ard(hipStream_t s, const double *dX, int n, int ldx, int D, const double *dy, const double *alpha,
                                  const double *ell, const double *sigma, int G, double jitter, double *Wall, double *d_out3,
                                  int *d_info_out, int *d_info_work)
{
    static_assert(SMALL_PTS_ARD == GPMI_SMALL_PTS_ARD, "batch size of the small-N ARD grid launch");
    SmallBatchArd b;
    for (int g = 0; g < G; ++g) {
        b.a2[g] = alpha[g] * alpha[g];
        b.diag[g] = sigma[g] * sigma[g] + jitter;
        for (int d = 0; d < GPMI_MAXD; ++d) b.inv_ell[g][d] = d < D ? 1.0 / ell[(size_t)g * D + d] : 0.0;
    }
    size_t ld, stride;
    small_ws_layout(n, &ld, &stride);
    launch_small<k_logml_small_batch_ard>(G, SMALL_LDS_DOUBLES, s, dX, n, ldx, D, dy, b, Wall,
                       stride, ld, d_out3, d_info_out, d_info_work, h_exp);
}

// G points (any number) whose parameters are uploaded to d_par (G * (2 + GPMI_MAXD) doubles) in stream order; ell: one
// length-scale per point (n_ell == 1) or D per point (point-major); Wall: G slices (small_ws_layout)
// count doubles of host memory into device memory in stream order, PUT_MAX per launch (the host array may be reused at once)
void launch_put_doubles(hipStream_t s, const double *src, size_t count, double *dst)
{
    PutArgs a;
    for (size_t i0 = 0; i0 < count; i0 += PUT_MAX) {
        const int nc = (count - i0 < (size_t)PUT_MAX) ? (int)(count - i0) : PUT_MAX;
        for (int i = 0; i < nc; ++i) a.v[i] = src[i0 + i];
        hipLaunchKernelGGL(k_put_doubles, dim3(1), 256, 0, s, a, dst + i0, nc);
    }
}

// the SMALL_PAR records of G points into d_par, in stream order
static void put_small_par(hipStream_t s, int D, const double *alpha, const double *ell, int n_ell, const double *sigma, int G,
                          double jitter, double *d_par)
{
    static_assert(PUT_MAX % SMALL_PAR == 0, "whole points per upload");
    PutArgs a;
    for (int g0 = 0; g0 < G; g0 += PUT_MAX / SMALL_PAR) {
        const int gc = (G - g0 < PUT_MAX / SMALL_PAR) ? G - g0 : PUT_MAX / SMALL_PAR;
        for (int g = 0; g < gc; ++g) {
            double *q = a.v + g * SMALL_PAR;
            q[0] = alpha[g0 + g] * alpha[g0 + g];
            q[1] = sigma[g0 + g] * sigma[g0 + g] + jitter;
            for (int d = 0; d < GPMI_MAXD; ++d)
                q[2 + d] = d < D ? 1.0 / (n_ell == 1 ? ell[g0 + g] : ell[(size_t)(g0 + g) * D + d]) : 0.0;
        }
        hipLaunchKernelGGL(k_put_doubles, dim3(1), 256, 0, s, a, d_par + (size_t)g0 * SMALL_PAR, gc * SMALL_PAR);
    }
}

void launch_logml_small_batch_dev(hipStream_t s, const double *dX, int n, int ldx, int D, const double *dy, const double *alpha,
                                  const double *ell, int n_ell, const double *sigma, int G, double jitter, double *d_par,
                                  double *Wall, double *d_out3, int *d_info_out, int *d_info_work)
{
    put_small_par(s, D, alpha, ell, n_ell, sigma, G, jitter, d_par);
    size_t ld, stride;
    small_ws_layout(n, &ld, &stride);
    launch_small<k_logml_small_batch_dev>(G, SMALL_LDS_DOUBLES, s, dX, n, ldx, D, dy, d_par, Wall,
                       stride, ld, d_out3, d_info_out, d_info_work, h_exp);
}

// value + gradient sums by one workgroup per point: W holds, per point, two slices of small_ws_layout (W, then U)
void launch_logml_grad_small(hipStream_t s, const double *dX, int n, int ldx, const double *dy, const SeParams &p, double diag_add,
                             double *W, double *d_res, int *d_info_out, int *d_info_work, double *stage, int *done, int seq)
{
    size_t ld, stride;
    small_ws_layout(n, &ld, &stride);
    launch_small<k_logml_grad_small>(1, SMALL_GRAD_LDS_DOUBLES, s, dX, n, ldx, dy, p, diag_add, W, ld,
                       W + stride, d_res, d_info_out, d_info_work, h_exp, stage, done, seq);
}

void launch_logml_grad_small_batch(hipStream_t s, const double *dX, int n, int ldx, int D, const double *dy, const double *alpha,
                                   const double *rho, const double *sigma, int G, double jitter, double *Wall, double *d_res,
                                   int *d_info_out, int *d_info_work, double *stage, int *done, int seq, int *arrive)
{
    const SmallBatch b = small_batch(alpha, rho, sigma, G, jitter);
    size_t ld, stride;
    small_ws_layout(n, &ld, &stride);
    launch_small<k_logml_grad_small_batch>(G, SMALL_GRAD_LDS_DOUBLES, s, dX, n, ldx, D, dy, b, Wall,
                       2 * stride, stride, ld, d_res, d_info_out, d_info_work, h_exp, stage, done, seq, arrive);
}

// G ARD points (any number; ell: G x D, point-major), `per` of them per launch: d_par holds G records, Wall 2 per slices
// (W, then U, per point) and d_info_work per ints; the launches of one call follow each other on s, so the slices are reused
void launch_logml_grad_batch_dev(hipStream_t s, const double *dX, int n, int ldx, int D, const double *dy, const double *alpha,
                                 const double *ell, const double *sigma, int G, double jitter, double *d_par, double *Wall, int per,
                                 double *d_res, int *d_info_out, int *d_info_work)
{
    put_small_par(s, D, alpha, ell, D, sigma, G, jitter, d_par);
    size_t ld, stride;
    small_ws_layout(n, &ld, &stride);
    for (int g0 = 0; g0 < G; g0 += per) {
        const int gc = (G - g0 < per) ? G - g0 : per;
        launch_small<k_logml_grad_batch_dev>(gc, SMALL_GRAD_LDS_DOUBLES, s, dX, n, ldx, D, dy, d_par + (size_t)g0 * SMALL_PAR, Wall,
                           2 * stride, stride, ld, d_res + (size_t)g0 * SMALL_GRAD_RES, d_info_out + g0, d_info_work, h_exp);
    }
}

// B draws by one workgroup each; Wall: B slices of small_ws_layout(n + m); dY: n x B, dZ, draws, mus: m x B (packed); d_par: 3 B
// doubles, d_info_work: 2 B ints
void launch_sample_derivs_small_batch(hipStream_t s, const double *dt, int n, const double *dts, int m, const double *dY,
                                      const double *params /* host: (l, a, sy) per draw */, int B, double jitter, const double *dZ,
                                      double *d_par, double *Wall, double *d_draws, double *d_mus, int *d_status, int *d_info_work)
{
    static_assert(PUT_MAX % 3 == 0, "whole draws per upload");
    PutArgs a;
    for (int g0 = 0; g0 < B; g0 += PUT_MAX / 3) {
        const int gc = (B - g0 < PUT_MAX / 3) ? B - g0 : PUT_MAX / 3;
        for (int q = 0; q < 3 * gc; ++q) a.v[q] = params[3 * (size_t)g0 + q];
        hipLaunchKernelGGL(k_put_doubles, dim3(1), 256, 0, s, a, d_par + 3 * (size_t)g0, 3 * gc);
    }
    size_t ld, stride;
    small_ws_layout(n + m, &ld, &stride);
    launch_small<k_sample_derivs_small_batch>(B, SMALL_LDS_DOUBLES, s, dt, n, dts, m, dY, d_par, jitter, dZ,
                       Wall, stride, ld, d_draws, d_mus, d_status, d_info_work);
}

void launch_gp_condition_small(hipStream_t s, const double *t, int n, const double *ts, int m, const double *y, int kindK, int kindS,
                               int kindSS, int compat, double a2, double l2, double s2, double jitter, double *W, double *Kn, size_t ldo,
                               double *mn, int *info_out, int *d_info_work, double *stage, int *done, int seq)
{
    size_t ld, stride;
    small_ws_layout(n + m, &ld, &stride);
    CondArgs q{kindK, kindS, kindSS, compat, a2, l2, s2, jitter};
    launch_small<k_gp_condition_small>(1, SMALL_LDS_DOUBLES, s, t, n, ts, m, y, q, W, ld, Kn, ldo, mn,
                       info_out, d_info_work, stage, done, seq);
}

void launch_gp_predict_small(hipStream_t s, const double *X, int n, int ldx, const double *Xs, int m, int ldxs, const double *y,
                             const SeParams &p, double diag_add, double *W, double *mean, double *var, int *info_out, int *d_info_work,
                             int *done, int seq)
{
    size_t ld, stride;
    small_ws_layout(n + m, &ld, &stride);
    launch_small<k_gp_predict_small>(1, SMALL_LDS_DOUBLES, s, X, n, ldx, Xs, m, ldxs, y, p, diag_add, W,
                       ld, mean, var, info_out, d_info_work, h_exp, done, seq);
}

void launch_gp_predict_joint_wg(hipStream_t s, const double *X, int n, int ldx, const double *Xs, int m, int ldxs, const double *y,
                                const SeParams &p, double diag_add, double post_jitter, double *W, double *mean, double *cov, size_t ldc,
                                const double *Z, int B, size_t ldz, double *draws, size_t ldd, int *info_out, int *d_info_work, int *done,
                                int seq)
{
    size_t ld, stride;
    small_ws_layout(n + m, &ld, &stride);
    launch_small<k_gp_predict_joint_wg>(1, SMALL_LDS_DOUBLES, s, X, n, ldx, Xs, m, ldxs, y, p, diag_add, post_jitter, W, ld, mean, cov,
                       ldc, Z, B, ldz, draws, ldd, info_out, d_info_work, h_exp, done, seq);
}

void launch_joint_predict_wg(hipStream_t s, const double *t, int n, const double *ts, int m, const double *yy, double a2, double l,
                             double s2, double jitter, int orders, const double *pj, double *W, double *mean, double *cov, size_t ldc,
                             const double *Z, int B, size_t ldz, double *draws, size_t ldd, int *info_out, int *d_info_work, int *done,
                             int seq)
{
    size_t ld, stride;
    const int p = __builtin_popcount(orders);
    small_ws_layout(2 * n + p * m, &ld, &stride);
    const JointPredArgs q = {a2, l * l, s2, jitter, pj[0], p > 1 ? pj[1] : 0.0, p > 2 ? pj[2] : 0.0, orders};
    launch_small<k_joint_predict_wg>(1, SMALL_LDS_DOUBLES, s, t, n, ts, m, yy, q, W, ld, mean, cov, ldc, Z, B, ldz, draws, ldd, info_out,
                       d_info_work, h_exp, done, seq);
}

void launch_exact_gp_small(hipStream_t s, const double *X, int n, int ldx, const double *z, const SeParams &p, double diag_add,
                           double *W, double *f, int *info_out, int *d_info_work, double *stage, int *done, int seq)
{
    size_t ld, stride;
    small_ws_layout(n, &ld, &stride);
    launch_small<k_exact_gp_small>(1, SMALL_LDS_DOUBLES, s, X, n, ldx, z, p, diag_add, W, ld, f, info_out,
                       d_info_work, h_exp, stage, done, seq);
}

// one workgroup; W: 4 slices of small_ws_layout(n) -- the covariance / factor, then [V | U | V] (3 n columns of the same ld)
void launch_exact_gp_vjp_small(hipStream_t s, const double *X, int n, int ldx, const SeParams &p, double diag_add, const double *Z, int k,
                               int ldz, const double *Fb, int ldfb, double *F, int ldf, double *Zb, int ldzb, double *W, double alpha,
                               const double *ell, int n_ell, double *grad, int *info_out, int *d_info_work, double *stage, int *done,
                               int seq)
{
    size_t ld, stride;
    small_ws_layout(n, &ld, &stride);
    const GradEll el = grad_ell(ell, n_ell);
    launch_small<k_exact_gp_vjp_small>(1, SMALL_LDS_DOUBLES, s, X, n, ldx, p, diag_add, Z, k, ldz, Fb,
                       ldfb, F, ldf, Zb, ldzb, W, W + stride, ld, alpha, el, n_ell, grad, info_out, d_info_work, h_exp, stage, done, seq);
}

// the same with a likelihood head between the product and the sweep (k <= 2); stage != null: n (D + k + m) doubles
void launch_latent_gp_small(hipStream_t s, const double *X, int n, int ldx, const SeParams &p, double diag_add, const double *Z, int k,
                            int ldz, const LatentHead &lh, double *out, double *Fb, int ldfb, double *F, int ldf, double *Zb, int ldzb,
                            double *W, double alpha, const double *ell, int n_ell, double *grad, int *info_out, int *d_info_work,
                            double *stage, int *done, int seq)
{
    size_t ld, stride;
    small_ws_layout(n, &ld, &stride);
    const GradEll el = grad_ell(ell, n_ell);
    launch_small<k_latent_gp_small>(1, SMALL_LDS_DOUBLES, s, X, n, ldx, p, diag_add, Z, k, ldz, lh, out,
                       Fb, ldfb, F, ldf, Zb, ldzb, W, W + stride, ld, alpha, el, n_ell, grad, info_out, d_info_work, h_exp, stage, done,
                       seq);
}

// one workgroup; W: 2 slices of small_ws_layout(n + k - 1) -- the covariance / factor with the k rows of F^T below, then U
void launch_centered_gp_small(hipStream_t s, const double *X, int n, int ldx, const SeParams &p, double diag_add, const double *F, int k,
                              int ldf, const LatentHead &lh, double *out, double *Fg, int ldfg, double *W, double alpha,
                              const double *ell, int n_ell, double *grad, int *info_out, int *d_info_work, double *stage, int *done,
                              int seq)
{
    size_t ld, stride;
    small_ws_layout(n + k - 1, &ld, &stride);
    const GradEll el = grad_ell(ell, n_ell);
    launch_small<k_centered_gp_small>(1, SMALL_LDS_DOUBLES, s, X, n, ldx, p, diag_add, F, k, ldf, lh,
                       out, Fg, ldfg, W, W + stride, ld, alpha, el, n_ell, grad, info_out, d_info_work, h_exp, stage, done, seq);
}

// P <= 64 length-scales, one workgroup each (n <= 128); Wall: 3 P slices of small_ws_layout(n)
void launch_rbf_cov_chol_small(hipStream_t s, const double *x, int n, const double *ls, int P, double *Wall, double *Lout, double *dLout,
                               size_t ostride, size_t ldo, int *info_out, int *d_info_work, double *stage)
{
    RbfBatch b;
    for (int p = 0; p < P; ++p) b.l[p] = ls[p];
    size_t ld, stride;
    small_ws_layout(n, &ld, &stride);
    launch_small<k_rbf_cov_chol_small>(P, SMALL_LDS_DOUBLES, s, x, n, b, Wall, stride, ld, Lout, dLout,
                       ostride, ldo, info_out, d_info_work, h_exp, stage);
}

// the factorisation alone by one workgroup (launch_potrf_partial at M <= tune.small_m)
void launch_potrf_small(hipStream_t s, double *W, size_t ld, int M, int ncol, int nfac, int *d_info)
{
    launch_small<k_potrf_small>(1, SMALL_LDS_DOUBLES, s, W, ld, M, ncol, nfac, d_info);
}

#ifdef GPMI_PROBES
// read and clear this translation unit's stamp arrays: the small kernels' phase stamps, and the cycles of the
// diagonal-block bodies they ran
int probe_small_read(hipStream_t s, unsigned long long *out8)
{
    unsigned long long z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (hipStreamSynchronize(s) != hipSuccess) return 1;
    if (hipMemcpyFromSymbol(out8, HIP_SYMBOL(g_small), 8 * sizeof(unsigned long long)) != hipSuccess) return 1;
    return hipMemcpyToSymbol(HIP_SYMBOL(g_small), z, sizeof z) != hipSuccess;
}

int probe_small_body_read(hipStream_t s, unsigned long long *out8)
{
    unsigned long long z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (hipStreamSynchronize(s) != hipSuccess) return 1;
    if (hipMemcpyFromSymbol(out8, HIP_SYMBOL(g_body), 8 * sizeof(unsigned long long)) != hipSuccess) return 1;
    return hipMemcpyToSymbol(HIP_SYMBOL(g_body), z, sizeof z) != hipSuccess;
}
#endif  // GPMI_PROBES
