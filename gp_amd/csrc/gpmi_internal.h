// Internal declarations shared by the libgpmi translation units (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/gpmi.h"

#define GPMI_NB 128          // inner panel width == diagonal-block order
#define GPMI_FPACK 9216      // doubles in one packed panel-factor buffer (36 tiles x 256)
#define GPMI_FPACK_SLOTS 16   // per-context ring of such buffers: one per 128-column panel of an outer block
#define GPMI_MAXD 8          // dimensions the register-resident fast path handles
#define GPMI_MAXD_BIG 64     // dimensions the generic path handles (inverse length-scales in kernel arguments)
#define GPMI_SMALL_PTS 128   // grid points per launch of the one-workgroup-per-point small-N kernel
#define GPMI_SMALL_PTS_ARD 32 // ... with a length-scale per dimension and point

typedef double d4 __attribute__((ext_vector_type(4)));

struct SeParams {            // squared-exponential hyper-parameters, kernel-argument resident
    double a2;               // alpha^2
    double inv_ell[GPMI_MAXD_BIG];
    int D;
};

// The caller's length-scales as a kernel argument (n_ell of them, zero beyond)
struct GradEll {
    double ell[GPMI_MAXD_BIG];
};
inline GradEll grad_ell(const double *ell, int n_ell)
{
    GradEll e;
    for (int d = 0; d < GPMI_MAXD_BIG; ++d) e.ell[d] = d < n_ell ? ell[d] : 0.0;
    return e;
}
// grad[0 .. n_ell] = (d/dalpha, d/dell...) from the contraction sums hs[0 .. D] of the gradient kernels: the one statement of
// every value + gradient entry point, on the host and in the finishing kernels.  Multiplications and one division, contraction
// off: the operation order is part of the results.
__host__ __device__ inline void gpmi_grad_from_sums(const double *hs, int D, double alpha, const double *ell, int n_ell, double *grad)
{
    grad[0] = 2.0 * hs[0] / alpha;
    if (n_ell == 1) {
        double t = 0.0;
        for (int d = 0; d < D; ++d) t += hs[1 + d];
        grad[1] = t / (ell[0] * ell[0] * ell[0]);
    } else {
        for (int d = 0; d < D; ++d) grad[1 + d] = hs[1 + d] / (ell[d] * ell[d] * ell[d]);
    }
}

// Algorithm switches of one context (gpmi_set_option).  Per context, never process-global: two
// contexts or two host threads do not change each other's algorithm; grid lanes copy their root's.
struct gpmi_tuning {
    int syrk_order;       // tile walk of multi-round trailing updates: 0 row-major, 2 XCD-partitioned bands
    int stagger;          // (mode << 16) | number of s_sleep(127) (~3.5 us each) for the late workgroup of a CU pair
    int fuse_diag;        // default 15; bit 0: in-block GEMMs, bit 1: trailing SYRK (multi-round), bit 2: sub-tiled diagonal tile, bit 3: single-round SYRK (sub-tiled)
    int nb_adapt;         // outer-block width re-chosen per block from the order of the matrix still to update
    int nb_thr[3];        // ... >= nb_thr[0]: 1024 columns, >= nb_thr[1]: 512, >= nb_thr[2]: 256, below: 128
    int ksplit, ksplit_max;
    int block_recursive;
    int debug_ncu;        // test hook: CU count the trailing-update planner sees instead of the device's (0: the device's); no kernel changes
    int se_nt;            // non-temporal stores in k_se_cov<>
    int small_n;          // grids of marginal likelihoods at n <= small_n (and D <= GPMI_MAXD): one workgroup per point, one launch (0: off)
    int small_n1;         // ... a single evaluation (or a grid of fewer than 6 points) up to this n: beyond it the multi-CU launch chain is faster
    int small_m;          // partial factorisation of <= small_m rows: one workgroup, one launch (0: off)
    int small_ng1, small_ng; // value + gradient by one workgroup: one evaluation up to n <= small_ng1, several (a sampler's chains) up to small_ng (<= 256; 0: off)
    int grad_aug_n, grad_aug_ng;  // gpmi_logml_grad / _grid: K^-1 and K^-1 y from one augmented partial factorisation up to this n (0: off)
    int small_vjp;           // gpmi_exact_gp_f_vjp[_dev]: one workgroup, one launch, up to n <= small_vjp (<= 256, D <= GPMI_MAXD, k <= GPMI_VJP_KMAX; 0: off)
    int small_cen;           // gpmi_centered_gp_lp_grad[_dev]: one workgroup, one launch, up to n <= small_cen (<= 256, D <= GPMI_MAXD, k <= GPMI_CEN_KMAX; 0: off)
    int small_gc;            // gpmi_gp_condition: one workgroup, one launch, up to n + m + 1 <= small_gc rows (0: off)
    int small_pr;            // gpmi_gp_predict[_dev]: one workgroup, one launch, up to n + m + 1 <= small_pr rows and D <= GPMI_MAXD (0: off)
    int predict_mb;          // gpmi_gp_predict / gpmi_seq_marginals: rows of Xs per chunk of the blocked chain (0: auto)
    int small_pj;            // gpmi_gp_predict_joint[_dev]: one workgroup, one launch, up to n + m + 1 <= small_pj rows and D <= GPMI_MAXD (0: off)
    int small_jp;            // gpmi_joint_predict[_dev]: one workgroup, one launch, up to 2n + p m + 1 <= small_jp rows (0: off)
    int small_sd, small_sdb; // sample_derivs_batch: one workgroup per draw when n + m + 1 <= small_sd rows and at least small_sdb (n + m + 1)^2 / 400^2 draws (0: off)
    int small_n2, small_g2;  // grids of >= small_g2 (n / 1024)^2 + 2 points: one workgroup per point up to n <= small_n2 (every CU a problem of its own)
};
void gpmi_tuning_defaults(gpmi_tuning *t);

struct gpmi_ctx {
    int device;
    int pid;
    gpmi_tuning tune;
    hipStream_t own_stream;
    hipStream_t stream;      // stream in use (own or caller's)
    // factorisation workspace: column-major, leading dimension ld, ncols columns (+ slack)
    double *W;
    size_t W_bytes;
    int ld, ncols;
    double *Fpack;           // packed factors of the current diagonal block
    double *scratch;         // small device scratch (results, staging)
    size_t scratch_bytes;
    int *d_info;
    int *d_ctr;              // zeroed counters: [0..2] persistent trailing update (tile, retired, early exits),
                             // [8] sub-tile counter of the fused in-block GEMM
    int ncu;                 // compute units of the device
    double *d_out;           // 3 doubles
    double *d_fin;           // slice sums of the finalize kernels
    double *h_pin;           // pinned, device-mapped host buffer: inputs and results of small host-buffer calls travel without a copy call
    double *h_pin_dev;       // its device address
    size_t h_pin_bytes;
    double *d_spar;          // device-parameter small-N grids: GPMI_SMALL_PAR doubles + one work int per point
    int *d_sinfo;
    int spar_pts;            // capacity (points)
    int pin_seq;             // sequence number of the completion flag in h_pin (one-launch host-buffer calls)
    // generic device staging buffers for the host-pointer API
    double *stage[4];
    size_t stage_bytes[4];
    int nb_outer;            // outer panel width (multiple of GPMI_NB)
    int timing;
    hipEvent_t ev[4];
    double last_ms[3];
    // per-kernel HIP-event timing (bench): category 0 covariance build, 1 trailing SYRK,
    // 2 panel kernels (diag potrf + panel solve + in-block update)
    int ktiming;
    void *ktimer;            // KTimer*
    // grid lanes: extra internal contexts (own workspace + streams) so that independent grid
    // points overlap -- one point's panel phase and SYRK tails run under another's bulk update
    int grid_lanes;          // 0 = auto
    // Cholesky-factor interpolation table (gpmi_interp_*): P stacked n x itp_ld matrices each
    double *itp_L, *itp_dL, *itp_part;
    double *itp_lp;          // host copy of the P length-scales
    int itp_P, itp_n;
    size_t itp_ld;
    // GP-regression lookup table (gpmi_interp_gp_*): P stacked lower triangles, ld itp-style, beside the Hermite table
    double *igp_M;
    double *igp_aux;         // device: lp (P) | LU of Sigma_P (P x P) | perm (P ints)
    double *igp_lp;          // host copy of the P knots
    int igp_P, igp_n;
    size_t igp_ld;
    double igp_rho;
    gpmi_ctx *lane[7];
    hipEvent_t evFork, evJoin;
    // Dispatch streams on distinct command-processor pipes (root context), found by probing:
    // kernels of two queues overlap freely only if the queues sit on different pipes
    // (see calibrate_streams in gpmi_api.hip).
    hipStream_t qstream[4];
    int nq;                  // number of mutually concurrent streams found (0 = not probed yet)
    int cal_want;            // ... the largest number a calibration run has searched for so far
    int lanes_active;        // inside a multi-lane call (grid, table build, batch): other lanes' kernels share the chip
    int calibrate;           // 1: run grid lanes on qstream[]; 0: on the lanes' plain streams
    // gpmi_logml_hess: the full S^-1, the weighted matrices K o R_d, the products P_d and the vectors of the second-order terms
    double *hess_buf;
    size_t hess_bytes;
};

// event-pair recorder; begin/end bracket one launch on the context's stream
void kt_begin(gpmi_ctx *c, int cat, hipStream_t s = nullptr);
void kt_end(gpmi_ctx *c, int cat, double work, hipStream_t s = nullptr, int flag = 0);

// ---- error plumbing -------------------------------------------------------
int gpmi_fail(int code, const char *fmt, ...);
#define HIPCHK(expr)                                                                   \
    do {                                                                               \
        hipError_t e_ = (expr);                                                        \
        if (e_ != hipSuccess)                                                          \
            return gpmi_fail(GPMI_EHIP, "%s failed: %s (%s:%d)", #expr,               \
                             hipGetErrorString(e_), __FILE__, __LINE__);               \
    } while (0)

// ---- kernel launchers (se_kernels.hip) -------------------------------------
// K (n x m, ldk) from device points; Y == X when dY == nullptr.
void launch_se_cov(const gpmi_ctx *c, hipStream_t s, const double *dX, int n, int ldx, const double *dY, int m, int ldy,
                   const SeParams &p, double diag_add, int lower, double *dK, size_t ldk);
void launch_deriv_cov(hipStream_t s, int kind, const double *dx, int n, const double *dy, int m,
                      double a2, double l, int compat, int lower, double *dK, size_t ldk);
void launch_deriv_elem(hipStream_t s, int kind, const double *tj, const double *tk, size_t len,
                       double l, double *out);
// joint 2n x 2n [[QQ+s2 I, QR],[RQ, RR]] + jitter I; lower != 0 writes i >= j only
void launch_joint_cov(hipStream_t s, const double *dt, int n, double a2, double l, double s2,
                      double jitter, int compat, int lower, double *dK, size_t ldk);
// star blocks of gpmi_joint_predict's workspace dW (order 2n + p m + 1, launch_joint_cov's S in its leading 2n x 2n block) for the
// p derivative orders in the bit mask `orders` (1 .. 7) at the m times dts: rows 2n + ia m + i hold a2 kind(a_ia, Q | R)(ts_i, t_j)
// in the columns j | n + j and a2 kind(a_ia, a_ib)(ts_i, ts_j) in the columns 2n + ib m + j, lower-stored; one exponential per
// pair of points, every entry with the bits of launch_deriv_cov for its kind
void launch_joint_star(hipStream_t s, const double *dt, int n, const double *dts, int m, int orders, double a2, double l, double *dW,
                       size_t ldw);
void launch_set_row(hipStream_t s, double *W, size_t ld, int row, const double *src, int n,
                    int ntotal);  // W[row, j] = j < n ? src[j] : 0, j < ntotal
void launch_copy_matrix(hipStream_t s, const double *src, size_t lds, double *dst, size_t ldd,
                        int rows, int cols, int mode);  // mode 0 full, 1 lower (upper zero), 2 lower->symmetric
void launch_add_diag(hipStream_t s, double *A, size_t ld, int n, double v);
void launch_transpose(hipStream_t s, const double *src, size_t lds, double *dst, size_t ldd, int rows, int cols);
void launch_hermite_blend(hipStream_t s, const double *L1, const double *L2, const double *D1, const double *D2,
                          size_t ld, int n, double x1, double x2, double l, double *out, size_t ldo);
void launch_hermite_mv(hipStream_t s, const double *L1, const double *L2, const double *D1, const double *D2,
                       size_t ld, int n, double x1, double x2, double l, const double *z, double *part, double *f,
                       double *dfdl /* nullable: (dv/dl) z, the reverse-mode partial of approx_Lz */);
int hermite_mv_chunks(int n);
#define GPMI_HMV_SMALL_N 256    // approx_Lz up to this n: one launch, z read straight from (possibly host-mapped) memory
// ---- reverse mode of the interpolated models (interp_kernels.hip) ----
// One pass over T stored lower triangles M_t (A = sum a_t M_t, B = sum b_t M_t): F = A Z (nullable), Zbar = A^T Fbar,
// lbar = sum_c Fbar[:,c]^T (B Z[:,c]); Fbar == nullptr: F alone.  k columns in groups of GPMI_TRI_KG; n <= GPMI_TRI_SMALL_N
// with k <= GPMI_TRI_KG is one launch of one workgroup (Z, Fbar, F, Zbar, lbar may be host-mapped), otherwise ws holds
// tri_vjp_ws_doubles(n, k) doubles.  Every reduction has a fixed order.
#define GPMI_TRI_KG 8
#define GPMI_TRI_SMALL_N 256
#define GPMI_GP_PMAX 64          // knots of the GP-regression lookup
bool tri_vjp_one_launch(int n, int k);
size_t tri_vjp_ws_doubles(int n, int k);
// Hermite model: the four triangles of the interval [x1, x2]; F bit-identical to launch_hermite_mv
void launch_hermite_vjp(hipStream_t s, const double *L1, const double *L2, const double *D1, const double *D2, size_t ld, int n,
                        double x1, double x2, double l, const double *Z, int ldz, const double *Fb, int ldfb, int k, double *F,
                        int ldf, double *Zb, int ldzb, double *lbar, double *ws);
// GP-regression model: P lookup triangles (stride ld * n), weights exp(-(l - lp_p)^2 / (2 rho^2)); lp on the device
void launch_gp_vjp(hipStream_t s, const double *M, size_t ld, int n, int P, const double *lp, double rho, double l,
                   const double *Z, int ldz, const double *Fb, int ldfb, int k, double *F, int ldf, double *Zb, int ldzb,
                   double *lbar, double *ws);
void launch_gp_blend(hipStream_t s, const double *M, size_t ld, int n, int P, const double *lp, double rho, double l,
                     double *out, size_t ldo);
// in place: the P stacked exact factors become lookup = (Sigma_P \ exact)^T; lu: row-major P x P partial-pivot LU
// factors, perm: the row taken at each step (device)
void launch_gp_lookup(hipStream_t s, double *M, size_t ld, int n, int P, const double *lu, const int *perm);
void launch_phi_mask(hipStream_t s, double *B, size_t ld, int n); // keep upper, halve diag, zero strict lower

// ---- kernel launchers (chol_kernels.hip): the blocked factorisation, solves and products --------------------
// Factor the first nfac columns of the M x ncol lower-stored matrix in W (right-looking,
// blocked); rows nfac..M-1 become L21 / the Schur complement of the trailing block.
int launch_potrf_partial(gpmi_ctx *c, double *W, size_t ld, int M, int ncol, int nfac, int *d_info,
                         double *Fpack_all /* nullable: keep every block's packed factors */);
// X <- X * L^-T for the rows [row0, M) of columns [0, n) using packed factors saved by a
// previous launch_potrf_partial(..., Fpack_all)
int launch_trsm_right(gpmi_ctx *c, const double *L, size_t ldl, int n, double *X, size_t ldx,
                      int mrows, const double *Fpack_all, int upper_tri = 0 /* 1: X upper triangular, 2: lower triangle of the result only */);
// C (lower tiles only) = A B^T for lower-triangular A and B the transpose of a lower-triangular matrix (n^3 / 3 flops)
void launch_gemm_tri_lower(hipStream_t s, const double *A, size_t lda, const double *B, size_t ldb, double *C, size_t ldc, int n);
// C (M x N) = beta_is_one ? C - A B^T : A B^T   (A: M x K, B: N x K, column-major)
void launch_gemm_nt(const gpmi_ctx *c, hipStream_t s, const double *A, size_t lda, const double *B, size_t ldb,
                    double *C, size_t ldc, int M, int N, int K, int accumulate_minus);
void launch_syrk_uut(const gpmi_ctx *c, hipStream_t s, const double *U, size_t ldu, double *C, size_t ldc, int n);
// C(lower) -= P P^T for a full n x n P (the general form of the trailing update's launch)
void launch_syrk_ppt(const gpmi_ctx *c, hipStream_t s, const double *P, size_t ldp, double *C, size_t ldc, int n);
void launch_pack_factors(hipStream_t s, const double *L, size_t ldl, int n, double *Fpack_all);
// ---- kernel launchers (loo_kernels.hip): leave-one-out cross-validation from -S^-1 (lower triangle, Wk) and +-S^-1 y (av) ----
// mu, var, lpd (n each, nullable), *loo, and the vectors of the gradient: ab[0 .. n) = a = asign av, u = a / d, sv = sqrt(v);
// NaN outputs when *info != 0
void launch_loo_points(hipStream_t s, const double *Wk, size_t ld, int n, const double *av, double asign, const double *y,
                       const int *info, double *mu, double *var, double *lpd, double *ab, double *u, double *sv, double *loo);
// M (n x n, both triangles, ldm) = S^-1 diag(sv) and b = S^-1 u; bpart: loo_bpart_doubles(n) doubles of scratch
size_t loo_bpart_doubles(int n);
void launch_loo_tiles(hipStream_t s, const double *Wk, size_t ld, int n, const double *u, const double *sv, double *M, size_t ldm,
                      double *bpart, double *b);
// grad (2 + n_ell) from the contraction sums (ns slots), NaN when *info != 0
void launch_loo_grad_finish(hipStream_t s, const double *sums, int D, int ns, double alpha, const double *ell, int n_ell, double sigma,
                            const int *info, double *grad);
// ---- kernel launchers (hess_kernels.hip): the Hessian of the log marginal likelihood from -S^-1 (lower triangle, Wk), +-S^-1 y
// (av, a = asign av) and the finished sums of the gradient's contraction (gsums, gns slots) ----
// doubles of the Hessian's own buffer (the full S^-1, n_ell weighted matrices, n_ell products, vectors, partial sums, record)
size_t hess_buf_doubles(int n, int n_ell);
// the result record inside that buffer: 3 + (2 + n_ell) + (2 + n_ell)^2 doubles for out3, grad and a packed hess
double *hess_record(double *buf, int n, int n_ell);
// hess (q x q, ldh, q = 2 + n_ell; both triangles, NaN when *info != 0), every launch on s
void launch_hess(const gpmi_ctx *c, hipStream_t s, double *buf, const double *X, int n, int ldx, const SeParams &p, double alpha,
                 const double *ell, int n_ell, double sigma, double diag_add, const double *y, const double *av, double asign,
                 const double *Wk, size_t ld, const double *gsums, int gns, const int *info, double *hess, int ldh);
// ---- kernel launchers (lowrank_kernels.hip): the Hermite-eigenfunction low-rank GP ------------------------------------------
// the scalars of one (scale, amp, l) the kernels build their recurrence coefficients from, kernel-argument resident
struct LrPar {
    double c0, dc0;   // psi_0 = c0 exp(-d2 x^2) and d c0 / d l
    double d2, dd2;   // delta^2 and its l-derivative
    double ab;        // alpha beta
    double pl;        // d log p_k / d l (the same for every column)
    double r, dr;     // eps^2 / (alpha^2 + delta^2 + eps^2) and its l-derivative
};
LrPar lr_params(double scale, double amp, double l);
void launch_lr_basis(hipStream_t s, const double *x, int n, int M, const LrPar &P, double *Phi, size_t ldp, double *dPhi /* nullable */,
                     size_t lddp);
// rows per chunk and chunks of the Gram kernel (functions of n and M alone), doubles of one partial, and of the whole scratch
// (partials and S) launch_lr_logml needs
int lr_gram_rows(int n, int M);
int lr_gram_chunks(int n, int M);
size_t lr_part_doubles(int M);
size_t lr_scratch_doubles(int n, int M);
// out3, grad (3, nullable) and *info of gpmi_lowrank_logml_grad: the Gram kernel, then the finishing kernel
void launch_lr_logml(hipStream_t s, const double *x, int n, const double *y, int M, const LrPar &P, double amp, double sigma,
                     double *scratch, double *out3, double *grad, int *info);
// gpmi_lowrank_latent_lp_grad; part: lr_latent_blocks(n) * (4 + M) doubles (unused by a single workgroup)
struct LatentHead;
int lr_latent_blocks(int n);
void launch_lr_latent(hipStream_t s, const double *x, int n, int M, const LrPar &P, double amp, const double *z, const LatentHead &lh,
                      double *q, double *qbar, double *part, double *out, double *zbar, double *grad);
// ---- kernel launchers (small_kernels.hip): a whole evaluation by ONE workgroup of one launch -----------------
// the partial factorisation alone (what launch_potrf_partial runs at M <= tune.small_m)
void launch_potrf_small(hipStream_t s, double *W, size_t ld, int M, int ncol, int nfac, int *d_info);
// small-N marginal likelihood: build + factorisation + solve + log-det by ONE workgroup per point
void small_ws_layout(int n, size_t *ld, size_t *stride);
void launch_logml_small(hipStream_t s, const double *dX, int n, int ldx, const double *dy, const SeParams &p, double diag_add,
                        double *W, size_t ld, double *d_out3, int *d_info_out, int *d_info_work,
                        double *stage /* nullable: device staging for host-mapped X, y */,
                        int *done = nullptr /* nullable: host-mapped completion flag, set to seq at the end */, int seq = 0);
void launch_logml_small_batch_ard(hipStream_t s, const double *dX, int n, int ldx, int D, const double *dy, const double *alpha,
                                  const double *ell /* G x D, point-major */, const double *sigma, int G, double jitter,
                                  double *Wall, double *d_out3, int *d_info_out, int *d_info_work);
void launch_logml_small_batch(hipStream_t s, const double *dX, int n, int ldx, int D, const double *dy, const double *alpha,
                              const double *rho, const double *sigma, int G, double jitter, double *Wall, double *d_out3,
                              int *d_info_out, int *d_info_work);
// value + gradient sums (GPMI_SMALL_GRAD_RES doubles per point: logml, sum log L_ii, z'z, then the GRAD_NS = 10 contraction
// sums) by one workgroup per point, n <= 256; the workspace holds TWO slices of small_ws_layout per point (W, then U = L^-T)
#define GPMI_SMALL_GRAD_RES (3 + 2 + GPMI_MAXD)
void launch_logml_grad_small(hipStream_t s, const double *dX, int n, int ldx, const double *dy, const SeParams &p, double diag_add,
                             double *W, double *d_res, int *d_info_out, int *d_info_work, double *stage, int *done = nullptr, int seq = 0);
void launch_logml_grad_small_batch(hipStream_t s, const double *dX, int n, int ldx, int D, const double *dy, const double *alpha,
                                   const double *rho, const double *sigma, int G, double jitter, double *Wall, double *d_res,
                                   int *d_info_out, int *d_info_work, double *stage = nullptr /* G n (D + 1) doubles: X, y host-mapped */,
                                   int *done = nullptr, int seq = 0, int *arrive = nullptr /* zeroed device int, left zero */);
// ... for any number of points with one length-scale per dimension each (ell: G x D, point-major), device data only: the
// parameters are uploaded to d_par (G * GPMI_SMALL_PAR doubles) in stream order, `per` <= GPMI_SMALL_GRAD_DEV_PTS points run per
// launch (Wall: 2 per slices, d_info_work: per ints), d_res: G records of GPMI_SMALL_GRAD_RES doubles
#define GPMI_SMALL_GRAD_DEV_PTS 128
void launch_logml_grad_batch_dev(hipStream_t s, const double *dX, int n, int ldx, int D, const double *dy, const double *alpha,
                                 const double *ell, const double *sigma, int G, double jitter, double *d_par, double *Wall, int per,
                                 double *d_res, int *d_info_out, int *d_info_work);
// count doubles from host memory to device memory in stream order, as kernel arguments (no staging buffer, no synchronisation)
void launch_put_doubles(hipStream_t s, const double *src, size_t count, double *dst);
// B posterior draws of the derivative process, one workgroup each (workspace: B slices of small_ws_layout(n + m); d_par: 3 B doubles,
// d_info_work: 2 B ints)
void launch_sample_derivs_small_batch(hipStream_t s, const double *dt, int n, const double *dts, int m, const double *dY,
                                      const double *params, int B, double jitter, const double *dZ, double *d_par, double *Wall,
                                      double *d_draws, double *d_mus, int *d_status, int *d_info_work);
// gp_condition by one workgroup (workspace: one slice of small_ws_layout(n + m)); t, ts, y / Kn, mn, info_out may be host-mapped (stage != null)
void launch_gp_condition_small(hipStream_t s, const double *t, int n, const double *ts, int m, const double *y, int kindK, int kindS,
                               int kindSS, int compat, double a2, double l2, double s2, double jitter, double *W, double *Kn, size_t ldo,
                               double *mn, int *info_out, int *d_info_work, double *stage, int *done = nullptr, int seq = 0);
// gp_predict by one workgroup (workspace: one slice of small_ws_layout(n + m), D <= GPMI_MAXD); every pointer but W and
// d_info_work may be host-mapped (each input is read once: no staging copy); var nullable
void launch_gp_predict_small(hipStream_t s, const double *X, int n, int ldx, const double *Xs, int m, int ldxs, const double *y,
                             const SeParams &p, double diag_add, double *W, double *mean, double *var, int *info_out, int *d_info_work,
                             int *done = nullptr, int seq = 0);
// gp_predict_joint by one workgroup (workspace: one slice of small_ws_layout(n + m), n + m <= 1023, D <= GPMI_MAXD; d_info_work: 2
// ints); every pointer but W and d_info_work may be host-mapped (each input is read once); cov nullable, Z / draws unused at B == 0
void launch_gp_predict_joint_wg(hipStream_t s, const double *X, int n, int ldx, const double *Xs, int m, int ldxs, const double *y,
                                const SeParams &p, double diag_add, double post_jitter, double *W, double *mean, double *cov, size_t ldc,
                                const double *Z, int B, size_t ldz, double *draws, size_t ldd, int *info_out, int *d_info_work,
                                int *done = nullptr, int seq = 0);
// gpmi_joint_predict by one workgroup (workspace: one slice of small_ws_layout(2n + p m), 2n + p m <= 1023; d_info_work: 2 ints);
// orders: bit mask of the p requested derivative orders, pj: their p post-jitters (host); every pointer but W and d_info_work
// may be host-mapped (each input is read once); cov nullable, Z / draws unused at B == 0
void launch_joint_predict_wg(hipStream_t s, const double *t, int n, const double *ts, int m, const double *yy, double a2, double l,
                             double s2, double jitter, int orders, const double *pj, double *W, double *mean, double *cov, size_t ldc,
                             const double *Z, int B, size_t ldz, double *draws, size_t ldd, int *info_out, int *d_info_work,
                             int *done = nullptr, int seq = 0);
// f = chol(K + diag_add I) z by one workgroup (n <= 256, D <= GPMI_MAXD); X, z / f, info_out may be host-mapped (stage != null)
void launch_exact_gp_small(hipStream_t s, const double *X, int n, int ldx, const double *z, const SeParams &p, double diag_add,
                           double *W, double *f, int *info_out, int *d_info_work, double *stage, int *done = nullptr, int seq = 0);
// the vector-Jacobian product of f = chol(K + diag_add I) z for k <= GPMI_VJP_KMAX columns by one workgroup (n <= 256,
// D <= GPMI_MAXD; workspace: 4 slices of small_ws_layout(n)).  Z, Fbar (inputs) and F (nullable), Zbar, grad (1 + n_ell), info_out
// may be host-mapped (stage != null: n (D + 2 k) doubles of device scratch)
#define GPMI_VJP_KMAX 8
void launch_exact_gp_vjp_small(hipStream_t s, const double *X, int n, int ldx, const SeParams &p, double diag_add, const double *Z, int k,
                               int ldz, const double *Fb, int ldfb, double *F, int ldf, double *Zb, int ldzb, double *W, double alpha,
                               const double *ell, int n_ell, double *grad, int *info_out, int *d_info_work, double *stage,
                               int *done = nullptr, int seq = 0);
// A likelihood head of gpmi_latent_gp_lp_grad: the m replicate columns of Y against the rows of F; sigma is read by
// GPMI_LIK_NORMAL alone
struct LatentHead {
    int family;        // GPMI_LIK_*
    const double *Y;   // n x m, leading dimension ldy
    int m, ldy;
    double sigma, log_sigma;   // log_sigma = log(sigma), formed on the host (NORMAL only)
};
// launch_exact_gp_vjp_small with the head between the product and the sweep (k <= 2): out[0] = lik, out[1] = d lik / d sigma,
// Fb (nullable) receives Fbar; stage != null: n (D + k + m) doubles of device scratch
void launch_latent_gp_small(hipStream_t s, const double *X, int n, int ldx, const SeParams &p, double diag_add, const double *Z, int k,
                            int ldz, const LatentHead &lh, double *out, double *Fb, int ldfb, double *F, int ldf, double *Zb, int ldzb,
                            double *W, double alpha, const double *ell, int n_ell, double *grad, int *info_out, int *d_info_work,
                            double *stage, int *done = nullptr, int seq = 0);
// gpmi_centered_gp_lp_grad by one workgroup (n <= 256, D <= GPMI_MAXD, k <= GPMI_CEN_KMAX; workspace: 2 slices of
// small_ws_layout(n + k - 1)): lh.family == GPMI_LIK_NONE: no head.  F, lh.Y (inputs) and out (4), Fg, grad (1 + n_ell), info_out
// may be host-mapped (stage != null: n (D + k + m) doubles of device scratch)
#define GPMI_CEN_KMAX 8
void launch_centered_gp_small(hipStream_t s, const double *X, int n, int ldx, const SeParams &p, double diag_add, const double *F, int k,
                              int ldf, const LatentHead &lh, double *out, double *Fg, int ldfg, double *W, double alpha,
                              const double *ell, int n_ell, double *grad, int *info_out, int *d_info_work, double *stage,
                              int *done = nullptr, int seq = 0);
// the chain's head (latent_kernels.hip): Fbar (n x k, ldfb) from F (n x k, ldf) and the head, one partial (lik, d lik / d sigma)
// pair per block of 256 rows in part (2 latent_head_blocks(n) doubles), added in index order into out[0..1] (NaN when *info != 0,
// and then Fbar is NaN too)
int latent_head_blocks(int n);
void launch_latent_head(hipStream_t s, const double *F, size_t ldf, int n, int k, const LatentHead &lh, double *Fb, size_t ldfb,
                        double *part, double *out, const int *info);
// rbf_cov_chol (L and dL/dl) for P <= 64 length-scales, one workgroup each, n <= 128 (workspace: 3 P slices of small_ws_layout(n));
// x / Lout, dLout, info_out may be host-mapped (stage != null: P n doubles of device scratch)
void launch_rbf_cov_chol_small(hipStream_t s, const double *x, int n, const double *ls, int P, double *Wall, double *Lout, double *dLout,
                               size_t ostride, size_t ldo, int *info_out, int *d_info_work, double *stage);
// any number of points, parameters uploaded to d_par (G * GPMI_SMALL_PAR doubles) in stream order; ell: one per point (n_ell == 1) or D per point
#define GPMI_SMALL_PAR (2 + GPMI_MAXD)
#define GPMI_SMALL_NMAX 1024   // n * D <= 9216: the scaled coordinates are staged in the workgroup's LDS
#define GPMI_SMALL_DEV_PTS 512 // points per launch of the device-parameter form (workspace slices held at a time)
void launch_logml_small_batch_dev(hipStream_t s, const double *dX, int n, int ldx, int D, const double *dy, const double *alpha,
                                  const double *ell, int n_ell, const double *sigma, int G, double jitter, double *d_par,
                                  double *Wall, double *d_out3, int *d_info_out, int *d_info_work);
// ---- kernel launchers (chol_kernels.hip): triangular helpers --------------------------------------------------
// inverses of L's 128 x 128 diagonal blocks (ceil(n / 128) x 128 x 128 doubles, tmp the same) from packed factors
void launch_diag_inverses(hipStream_t s, const double *Fpack_all, int n, double *Dinv, double *tmp);
// t = L^-1 k for ONE right-hand side in one launch (k_trsv_wave); k and t are different buffers of n doubles
int launch_trsv_lower(hipStream_t s, const double *L, size_t ldl, int n, const double *k, double *t, const double *Dinv,
                      int *ticket /* zeroed device int of the calling context (d_ctr + 32) */);
void launch_get_row(hipStream_t s, const double *W, size_t ld, int row, int col0, int m, double scale, double *out);
void launch_logml_finalize(hipStream_t s, const double *W, size_t ld, int n, int zrow,
                           const int *d_info, double *d_out3, int *d_info_out, double *part /* 2 ceil(n/256) doubles */);
int trmv_lower_chunks(int n);
void launch_trmv_lower(hipStream_t s, const double *L, size_t ldl, int n, const double *z, double *f,
                       double *part /* trmv_lower_chunks(n) * n doubles */);
// w = L^T u for k columns (u: n x k, ldu; w: n x k, ldw), fixed-order reductions (k_trmv_lower_t)
void launch_trmv_lower_t(hipStream_t s, const double *L, size_t ldl, int n, const double *u, size_t ldu, double *w, size_t ldw, int k);
#ifdef GPMI_PROBES
void launch_syrk_probe(const gpmi_ctx *c, hipStream_t s, const double *P, size_t ldp, double *C, size_t ldc, int m, int k);
void launch_probe_mfma(hipStream_t s, const double *A, const double *B, double *D);
void launch_probe_peak(hipStream_t s, double *sink, int iters, int *blocks, int *threads);
#endif

// ---- kernel launchers (predict_kernels.hip): the ends of the prediction chains ------------------------------
#define GPMI_PRED_SLICE 512      // columns of T per partial sum of the fused row reduction
#define GPMI_PRED_KSLICE 256     // training points per partial sum of the fused build-and-contract kernel
#define GPMI_PRED_BWD 64         // block order of the backward substitution
// doubles of `part` the two reductions need for mrows rows / m test points against n columns / training points
size_t predict_rows_part_doubles(int n, int mrows);
size_t predict_mean_part_doubles(int n, int m);
// mean[j] = T_j . v and var[j] = base - T_j . U_j over the n columns of the rows j < mrows of T (ldt) and U (ldu; U == T gives
// the squared norm), v[i * vstride]; slice partials, then their sum in slice order: identical bits on every call.  info
// (nullable, device): non-zero -> NaN outputs; info_out (nullable) receives it.  var nullable.
void launch_predict_rows(hipStream_t s, const double *T, size_t ldt, const double *U, size_t ldu, const double *v, size_t vstride,
                         int n, int mrows, double base, double *part, double *mean, double *var, const int *info, int *info_out);
// a = L^-T z (z: n contiguous doubles, overwritten with intermediate values; a: n doubles) by a chain of one launch per block
// of GPMI_PRED_BWD columns, last block first: diagonal-block back-substitution by one wave, then z[0 .. k0) -= L[k, 0 .. k0)^T a_k
// by wave-wide sums of a fixed shape
void launch_trsv_lower_t(hipStream_t s, const double *L, size_t ldl, int n, double *z, double *a);
// mean[j] = sum_i k(xs_j, x_i) a_i without storing the cross-covariance: entries as gpmi_se_cov writes them
void launch_predict_mean(hipStream_t s, const double *X, int n, int ldx, const double *Xs, int m, int ldxs, const SeParams &p,
                         const double *a, double *part, double *mean, const int *info, int *info_out);
// read-out of the joint posterior's chain: S (m x m, lower, ld) is the Schur block, row[r * ld] = -mean[r].  mean is written,
// post_jitter is added to the diagonal of S IN PLACE, and cov (nullable; ldc) receives S mirrored; *info != 0 -> NaN outputs
void launch_joint_readout(hipStream_t s, double *S, size_t ld, const double *row, int m, double post_jitter, double *mean, double *cov,
                          size_t ldc, const int *info);
// ... with one post_jitter per block of mb rows (at most three blocks: m <= 3 mb): row r takes pj[r / mb]
void launch_joint_readout_blocks(hipStream_t s, double *S, size_t ld, const double *row, int m, const double *pj, int mb, double *mean,
                                 double *cov, size_t ldc, const int *info);
// draws = mean 1^T + L Z for the m x m lower-triangular L (ldl; its strict upper part is never read) and B columns (Z: ldz,
// draws: ldd), one MFMA product; a column's bits do not depend on B or on the other columns.  *info_a or *info_b (nullable)
// non-zero -> every draw is NaN
void launch_tril_draws(hipStream_t s, const double *L, size_t ldl, int m, const double *mean, const double *Z, size_t ldz, int B,
                       double *draws, size_t ldd, const int *info_a, const int *info_b);
