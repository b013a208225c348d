// Exact Hessian of the GP log marginal likelihood in theta = (alpha, ell.., sigma) (gpmi_logml_hess; gfx950 only): everything
// behind the factorisation chain, which leaves -A = -S^-1 (lower triangle) and a = S^-1 y on the device, and behind the
// gradient's own contraction.  With S = K + s I, G = (a a' - A) / 2, S_i = dS/dtheta_i, b_i = S_i a, P_i = A S_i:
//   H_ij = <G, S_ij> - b_i' A b_j + 1/2 sum_kl P_i[k,l] P_j[l,k]                                   
//   S_alpha = (2 / alpha) K, S_sigma = 2 sigma I, S_ell_d = K o R_d, R_d = r_d^2 / ell_d^3 (one length-scale: sum_d r_d^2 / ell^3).
// Only the n_ell matrices P_d = A (K o R_d) are products (k_gemm_nt, unchanged); P_alpha = (2 / alpha) (I - s A) and
// P_sigma = 2 sigma A turn their traces into tr A, |A|_F^2, tr P_d and tr(A P_d), and b_alpha = (2 / alpha) (y - s a),
// b_sigma = 2 sigma a are closed forms.  Every sum has a fixed shape and order: no atomics, repeated calls give identical bits.
#include "gpmi_internal.h"

namespace {

constexpr int HESS_PITCH = 65;                              // row pitch of a 64 x 64 tile in LDS (transposed reads without bank conflicts)
constexpr int HESS_Q = 2 + GPMI_MAXD;                       // the most hyper-parameters
constexpr int HESS_NS = GPMI_MAXD * (GPMI_MAXD + 1) / 2;    // second-order slots per tile: the pairs d <= e
constexpr int HESS_CH = 256;                                // columns per chunk of the multi-vector product

// slot of the pair (d, e), d <= e < m, among the m (m + 1) / 2 pairs, row by row
__host__ __device__ inline int hess_pair(int d, int e, int m) { return d * m - d * (d - 1) / 2 + (e - d); }

// One 64 x 64 tile (rt, ct) of the n_ell weighted matrices K o R_d, regenerated from X: thread = one row x 16 columns.  The
// matrices are symmetric and a mirror tile is computed, not transposed: (x_i - x_j)^2 has the bits of (x_j - x_i)^2.
//   Sm[d][i, j] = kse_ij R_d[i, j];   bpart[d][4 ct + grp][i] = sum over the thread's 16 columns of Sm[d][i, j] a_j
__device__ inline void hess_se_tile(int rt, int ct, int lane, int grp, const double *__restrict__ X, int n, int ldx, const SeParams &p,
                                    int m, const double *__restrict__ av, double asign, double *__restrict__ Sm, size_t ldm,
                                    size_t mstride, double *__restrict__ bpart, int T)
{
    const int i = rt * 64 + lane;
    double acc[GPMI_MAXD];
#pragma unroll
    for (int d = 0; d < GPMI_MAXD; ++d) acc[d] = 0.0;
    if (i < n) {
        for (int q = 0; q < 16; ++q) {
            const int j = ct * 64 + grp * 16 + q;
            if (j >= n) break;
            const double aj = asign * av[j];
            if (m == 1) {   // one length-scale, any D
                double R = 0.0;
                for (int d = 0; d < p.D; ++d) {
                    const double r = X[(size_t)i + (size_t)d * ldx] - X[(size_t)j + (size_t)d * ldx];
                    R += r * r;
                }
                const double ie = p.inv_ell[0];
                const double v = p.a2 * exp(-0.5 * (R * ie * ie)) * (R * ie * ie * ie);
                Sm[(size_t)i + (size_t)j * ldm] = v;
                acc[0] += v * aj;
            } else {        // one per dimension, D = m <= GPMI_MAXD
                double r2[GPMI_MAXD], e = 0.0;
#pragma unroll
                for (int d = 0; d < GPMI_MAXD; ++d) {
                    const double r = d < m ? X[(size_t)i + (size_t)d * ldx] - X[(size_t)j + (size_t)d * ldx] : 0.0;
                    r2[d] = r * r;
                    e += r2[d] * p.inv_ell[d] * p.inv_ell[d];
                }
                const double kse = p.a2 * exp(-0.5 * e);
#pragma unroll
                for (int d = 0; d < GPMI_MAXD; ++d)
                    if (d < m) {
                        const double v = kse * (r2[d] * p.inv_ell[d] * p.inv_ell[d] * p.inv_ell[d]);
                        Sm[(size_t)d * mstride + (size_t)i + (size_t)j * ldm] = v;
                        acc[d] += v * aj;
                    }
            }
        }
    }
    const size_t npad = (size_t)T * 64;
#pragma unroll
    for (int d = 0; d < GPMI_MAXD; ++d)
        if (d < m) bpart[((size_t)d * 4 * T + (size_t)ct * 4 + grp) * npad + (size_t)rt * 64 + lane] = acc[d];
}

// One tile (ti, tj), tj <= ti, of the lower triangle of Wk = -A: A as a full symmetric matrix (the tile above the diagonal is
// the transposed tile, read through LDS so that both stores run along columns), then the tile and its mirror image of the
// weighted matrices with their parts of b_d = (K o R_d) a.
__global__ __launch_bounds__(256) void k_hess_operands(const double *__restrict__ X, int n, int ldx, SeParams p, int m,
                                                       const double *__restrict__ av, double asign, const double *__restrict__ Wk,
                                                       size_t ld, double *__restrict__ Af, double *__restrict__ Sm, size_t ldm,
                                                       size_t mstride, double *__restrict__ bpart)
{
    __shared__ double sa[64 * HESS_PITCH];
    const int ti = blockIdx.x, tj = blockIdx.y, T = gridDim.x;
    if (tj > ti) return;
    const int lane = threadIdx.x & 63, grp = threadIdx.x >> 6;
    const bool diag = ti == tj;
    {   // sa[c][r] = A[64 ti + r, 64 tj + c] where the lower triangle holds it, 0 elsewhere
        const int i = ti * 64 + lane;
        for (int cc = grp; cc < 64; cc += 4) {
            const int j = tj * 64 + cc;
            sa[cc * HESS_PITCH + lane] = (i < n && j < n && j <= i) ? -Wk[(size_t)i + (size_t)j * ld] : 0.0;
        }
    }
    __syncthreads();
    {
        const int i = ti * 64 + lane;
        for (int q = 0; q < 16; ++q) {
            const int c = grp * 16 + q, j = tj * 64 + c;
            const double v = (diag && c > lane) ? sa[lane * HESS_PITCH + c] : sa[c * HESS_PITCH + lane];
            if (i < n && j < n) Af[(size_t)i + (size_t)j * ldm] = v;
        }
    }
    if (!diag) {
        const int j = tj * 64 + lane;   // row of the mirror tile
        for (int q = 0; q < 16; ++q) {
            const int r = grp * 16 + q, i = ti * 64 + r;
            if (i < n && j < n) Af[(size_t)j + (size_t)i * ldm] = sa[lane * HESS_PITCH + r];
        }
    }
    hess_se_tile(ti, tj, lane, grp, X, n, ldx, p, m, av, asign, Sm, ldm, mstride, bpart, T);
    if (!diag) hess_se_tile(tj, ti, lane, grp, X, n, ldx, p, m, av, asign, Sm, ldm, mstride, bpart, T);
}

// The q = 2 + m vectors b_i = S_i a, one column each of Bv (n x q): b_alpha = (2 / alpha) (y - s a), b_ell_d = the 4 T slots of
// row i added in slot order, b_sigma = 2 sigma a
__global__ __launch_bounds__(256) void k_hess_bsum(const double *__restrict__ bpart, int T, int n, int m, const double *__restrict__ av,
                                                   double asign, const double *__restrict__ y, double s, double alpha, double sigma,
                                                   double *__restrict__ Bv)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const size_t npad = (size_t)T * 64;
    const double a = asign * av[i];
    Bv[i] = (2.0 / alpha) * (y[i] - s * a);
    for (int d = 0; d < m; ++d) {
        double acc = 0.0;
        for (int t = 0; t < 4 * T; ++t) acc += bpart[((size_t)d * 4 * T + t) * npad + i];
        Bv[(size_t)(1 + d) * n + i] = acc;
    }
    Bv[(size_t)(1 + m) * n + i] = 2.0 * sigma * a;
}

// cpart[chunk][j][i] = sum over the chunk's HESS_CH columns l, in index order, of A[i, l] Bv[l, j]: thread = one row, q columns
__global__ __launch_bounds__(256) void k_hess_mv_part(const double *__restrict__ Af, size_t ldm, int n, const double *__restrict__ Bv,
                                                      int q, double *__restrict__ cpart)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int c0 = blockIdx.y * HESS_CH, c1 = c0 + HESS_CH < n ? c0 + HESS_CH : n;
    double acc[HESS_Q];
#pragma unroll
    for (int j = 0; j < HESS_Q; ++j) acc[j] = 0.0;
    for (int l = c0; l < c1; ++l) {
        const double a = Af[(size_t)i + (size_t)l * ldm];
#pragma unroll
        for (int j = 0; j < HESS_Q; ++j)
            if (j < q) acc[j] += a * Bv[(size_t)j * n + l];
    }
#pragma unroll
    for (int j = 0; j < HESS_Q; ++j)
        if (j < q) cpart[((size_t)blockIdx.y * q + j) * n + i] = acc[j];
}

// Cv (n x q) = A Bv: the chunks added in chunk order
__global__ __launch_bounds__(256) void k_hess_mv_sum(const double *__restrict__ cpart, int n, int nchunk, int q, double *__restrict__ Cv)
{
    const int i = blockIdx.x * 256 + threadIdx.x, j = blockIdx.y;
    if (i >= n) return;
    double acc = 0.0;
    for (int ch = 0; ch < nchunk; ++ch) acc += cpart[((size_t)ch * q + j) * n + i];
    Cv[(size_t)j * n + i] = acc;
}

// fixed-shape tree over the 256 threads of a workgroup; the result is valid in thread 0
__device__ inline double hess_tree256(double *red, double v)
{
    red[threadIdx.x] = v;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}

// dots[i + j q] = b_i' c_j for i <= j: one workgroup per pair, stride-256 partial sums, then one tree
__global__ __launch_bounds__(256) void k_hess_dots(const double *__restrict__ Bv, const double *__restrict__ Cv, int n, int q,
                                                   double *__restrict__ dots)
{
    __shared__ double red[256];
    const int i = blockIdx.x, j = blockIdx.y;
    if (i > j) return;
    double acc = 0.0;
    for (int l = threadIdx.x; l < n; l += 256) acc += Bv[(size_t)i * n + l] * Cv[(size_t)j * n + l];
    const double r = hess_tree256(red, acc);
    if (threadIdx.x == 0) dots[i + j * q] = r;
}

// The second-order contraction, the tile walk of the gradient's k_grad_partial (64 x 64 tiles of the lower triangle, thread =
// one row x 16 columns, g = (a_i a_j + W_ij) / 2 with W = -A, w = 2 off the diagonal): per tile the HESS_NS sums of
// w g kse r_d^2 r_e^2, d <= e (slot hess_pair(d, e, GPMI_MAXD)); one length-scale per dimension, D <= GPMI_MAXD
__global__ __launch_bounds__(256) void k_hess_second_ard(const double *__restrict__ X, int n, int ldx, SeParams p,
                                                         const double *__restrict__ a, const double *__restrict__ W, size_t ld,
                                                         double *__restrict__ part)
{
    __shared__ double red[256];
    const int ti = blockIdx.x, tj = blockIdx.y;
    if (tj > ti) return;
    const int i = ti * 64 + (threadIdx.x & 63);
    const int jbase = tj * 64 + (threadIdx.x >> 6) * 16;
    double acc[HESS_NS];
#pragma unroll
    for (int s = 0; s < HESS_NS; ++s) acc[s] = 0.0;
    if (i < n) {
        double xi[GPMI_MAXD];
#pragma unroll
        for (int d = 0; d < GPMI_MAXD; ++d) xi[d] = d < p.D ? X[(size_t)i + (size_t)d * ldx] : 0.0;
        const double ai = a[i];
        for (int q = 0; q < 16; ++q) {
            const int j = jbase + q;
            if (j >= n || j > i) break;
            double e = 0.0, r2[GPMI_MAXD];
#pragma unroll
            for (int d = 0; d < GPMI_MAXD; ++d) {
                const double r = d < p.D ? xi[d] - X[(size_t)j + (size_t)d * ldx] : 0.0;
                r2[d] = r * r;
                e += r2[d] * p.inv_ell[d] * p.inv_ell[d];
            }
            const double g = 0.5 * (ai * a[j] + W[(size_t)i + (size_t)j * ld]);
            const double c = ((i == j) ? 1.0 : 2.0) * g * (p.a2 * exp(-0.5 * e));
#pragma unroll
            for (int d = 0; d < GPMI_MAXD; ++d) {
                const double cd = c * r2[d];
#pragma unroll
                for (int f = d; f < GPMI_MAXD; ++f) acc[hess_pair(d, f, GPMI_MAXD)] += cd * r2[f];
            }
        }
    }
    const size_t slot = ((size_t)ti * (ti + 1) / 2 + tj) * HESS_NS;
#pragma unroll
    for (int s = 0; s < HESS_NS; ++s) {
        const double r = hess_tree256(red, acc[s]);
        if (threadIdx.x == 0) part[slot + s] = r;
    }
}

// ... with ONE length-scale and any D <= GPMI_MAXD_BIG: one slot per tile, the sum of w g kse (sum_d r_d^2)^2
__global__ __launch_bounds__(256) void k_hess_second_iso(const double *__restrict__ X, int n, int ldx, SeParams p,
                                                         const double *__restrict__ a, const double *__restrict__ W, size_t ld,
                                                         double *__restrict__ part)
{
    __shared__ double red[256];
    const int ti = blockIdx.x, tj = blockIdx.y;
    if (tj > ti) return;
    const int i = ti * 64 + (threadIdx.x & 63);
    const int jbase = tj * 64 + (threadIdx.x >> 6) * 16;
    double acc = 0.0;
    if (i < n) {
        const double ai = a[i], ie = p.inv_ell[0];
        for (int q = 0; q < 16; ++q) {
            const int j = jbase + q;
            if (j >= n || j > i) break;
            double R = 0.0;
            for (int d = 0; d < p.D; ++d) {
                const double r = X[(size_t)i + (size_t)d * ldx] - X[(size_t)j + (size_t)d * ldx];
                R += r * r;
            }
            const double g = 0.5 * (ai * a[j] + W[(size_t)i + (size_t)j * ld]);
            acc += ((i == j) ? 1.0 : 2.0) * g * (p.a2 * exp(-0.5 * (R * ie * ie))) * (R * R);
        }
    }
    const double r = hess_tree256(red, acc);
    if (threadIdx.x == 0) part[(size_t)ti * (ti + 1) / 2 + tj] = r;
}

// Pair traces over the m1 = n_ell + 1 full matrices M_0 .. M_{m1 - 1} = P_0, .., A (mstride apart): workgroup (I, J, z) takes
// the pair (d, e), d <= e, number z and the 64 x 64 tile (I, J) of M_d with the tile (J, I) of M_e, read along columns into
// LDS and used transposed.  Per tile two slots: [0] sum_kl M_d[k, l] M_e[l, k], [1] the tile's part of tr M_d (d == e, I == J).
__global__ __launch_bounds__(256) void k_hess_traces(const double *__restrict__ M, size_t ldm, size_t mstride, int n, int m1,
                                                     double *__restrict__ tpart)
{
    __shared__ double sa[64 * HESS_PITCH], red[256];
    const int I = blockIdx.x, J = blockIdx.y, T = gridDim.x;
    int d = 0, e = 0;
    {
        int z = blockIdx.z;
        for (d = 0; d < m1; ++d) {
            if (z < m1 - d) {
                e = d + z;
                break;
            }
            z -= m1 - d;
        }
    }
    const double *Md = M + (size_t)d * mstride, *Me = M + (size_t)e * mstride;
    const int lane = threadIdx.x & 63, grp = threadIdx.x >> 6;
    {   // sa[c][r] = M_e[64 J + r, 64 I + c]
        const int l = J * 64 + lane;
        for (int cc = grp; cc < 64; cc += 4) {
            const int k = I * 64 + cc;
            sa[cc * HESS_PITCH + lane] = (l < n && k < n) ? Me[(size_t)l + (size_t)k * ldm] : 0.0;
        }
    }
    __syncthreads();
    const int k = I * 64 + lane;
    double acc = 0.0;
    if (k < n)
        for (int q = 0; q < 16; ++q) {
            const int lc = grp * 16 + q, l = J * 64 + lc;
            if (l >= n) break;
            acc += Md[(size_t)k + (size_t)l * ldm] * sa[lane * HESS_PITCH + lc];
        }
    const double tr = (d == e && I == J && grp == 0 && k < n) ? Md[(size_t)k + (size_t)k * ldm] : 0.0;
    const size_t slot = (((size_t)blockIdx.z * T + I) * T + J) * 2;
    const double r0 = hess_tree256(red, acc);
    const double r1 = hess_tree256(red, tr);
    if (threadIdx.x == 0) {
        tpart[slot] = r0;
        tpart[slot + 1] = r1;
    }
}

// sums[b ns + s] = the ntiles slots s of group b (gstride doubles apart), stride 1024 per thread, then one tree
__global__ __launch_bounds__(1024) void k_hess_sum(const double *__restrict__ part, size_t gstride, size_t ntiles, int ns,
                                                   double *__restrict__ sums)
{
    __shared__ double red[1024];
    const double *pt = part + (size_t)blockIdx.x * gstride;
    for (int s = 0; s < ns; ++s) {
        double acc = 0.0;
        for (size_t t = threadIdx.x; t < ntiles; t += 1024) acc += pt[t * (size_t)ns + s];
        red[threadIdx.x] = acc;
        __syncthreads();
        for (int h = 512; h > 0; h >>= 1) {
            if ((int)threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
            __syncthreads();
        }
        if (threadIdx.x == 0) sums[(size_t)blockIdx.x * ns + s] = red[0];
        __syncthreads();
    }
}

struct HessFinish {
    double alpha, sigma, s;   // s = sigma^2 + jitter
    GradEll e;
    int n, D, m, gns;         // gns: slots of the gradient's sums (c0, c_d .., tr G)
};

// H from the sums: gs the gradient's (sum w g kse, sum w g kse r_d^2, tr G), hs the second-order ones, ts the pair traces
// (two per pair), dots the b_i' c_j.  Each entry is computed once, for i <= j, and written to both triangles; NaN when
// *info != 0.
__global__ void k_hess_finish(const double *__restrict__ gs, const double *__restrict__ hs, const double *__restrict__ ts,
                              const double *__restrict__ dots, HessFinish f, const int *__restrict__ info, double *__restrict__ hess,
                              int ldh)
{
    if (threadIdx.x != 0) return;
    const int m = f.m, q = 2 + m, m1 = m + 1;
    if (*info != 0) {
        for (int j = 0; j < q; ++j)
            for (int i = 0; i < q; ++i) hess[(size_t)i + (size_t)j * ldh] = __builtin_nan("");
        return;
    }
    const double alpha = f.alpha, sigma = f.sigma, s = f.s;
    const double c0 = gs[0], trG = gs[f.gns - 1];
    const double fA = ts[2 * hess_pair(m, m, m1)], tA = ts[2 * hess_pair(m, m, m1) + 1];
    double call = 0.0;   // one length-scale: sum_d of the per-dimension sums
    for (int d = 0; d < f.D; ++d) call += gs[1 + d];
    for (int j = 0; j < q; ++j)
        for (int i = 0; i <= j; ++i) {
            double t1, t3;   // <G, S_ij> and the trace term
            if (j == 0) {                      // (alpha, alpha)
                t1 = 2.0 * c0 / (alpha * alpha);
                t3 = (2.0 / (alpha * alpha)) * (((double)f.n - 2.0 * s * tA) + s * s * fA);
            } else if (j <= m && i == 0) {     // (alpha, ell_d)
                const int d = j - 1;
                const double l = f.e.ell[d], cd = m == 1 ? call : gs[1 + d];
                t1 = (2.0 / alpha) * (cd / (l * l * l));
                t3 = (ts[2 * hess_pair(d, d, m1) + 1] - s * ts[2 * hess_pair(d, m, m1)]) / alpha;
            } else if (j <= m) {               // (ell_d, ell_e), d <= e
                const int d = i - 1, e = j - 1;
                const double ld_ = f.e.ell[d], le = f.e.ell[e];
                const double h2 = m == 1 ? hs[0] : hs[hess_pair(d, e, GPMI_MAXD)];
                t1 = h2 / ((ld_ * ld_ * ld_) * (le * le * le));
                if (d == e) t1 -= 3.0 * (m == 1 ? call : gs[1 + d]) / ((ld_ * ld_) * (ld_ * ld_));
                t3 = 0.5 * ts[2 * hess_pair(d, e, m1)];
            } else if (i == 0) {               // (alpha, sigma)
                t1 = 0.0;
                t3 = (2.0 * sigma / alpha) * (tA - s * fA);
            } else if (i <= m) {               // (ell_d, sigma)
                t1 = 0.0;
                t3 = sigma * ts[2 * hess_pair(i - 1, m, m1)];
            } else {                           // (sigma, sigma)
                t1 = 2.0 * trG;
                t3 = 2.0 * sigma * sigma * fA;
            }
            const double h = (t1 - dots[i + j * q]) + t3;
            hess[(size_t)i + (size_t)j * ldh] = h;
            hess[(size_t)j + (size_t)i * ldh] = h;
        }
}

struct HessLayout {
    size_t ldm, mstride;                                          // the n x n matrices: leading dimension, distance
    size_t S, P, A, Bv, Cv, bpart, cpart, hpart, tpart, sums, rec, total;   // offsets in doubles
};

HessLayout hess_layout(int n, int m)
{
    HessLayout L;
    const size_t T = (size_t)((n + 63) / 64), q = (size_t)(2 + m), nchunk = (size_t)((n + HESS_CH - 1) / HESS_CH);
    const size_t npairs = (size_t)(m + 1) * (m + 2) / 2;
    L.ldm = (size_t)(((n + 15) / 16) * 16 + 16);
    L.mstride = L.ldm * (size_t)n;
    L.S = 0;
    L.P = (size_t)m * L.mstride;     // P_0 .. P_{m - 1}, A: the m + 1 matrices of the pair traces, in this order
    L.A = 2 * (size_t)m * L.mstride;
    L.Bv = (2 * (size_t)m + 1) * L.mstride + L.ldm;
    L.Cv = L.Bv + q * n;
    L.bpart = L.Cv + q * n;
    L.cpart = L.bpart + (size_t)m * 4 * T * (T * 64);
    L.hpart = L.cpart + nchunk * q * n;
    L.tpart = L.hpart + T * (T + 1) / 2 * HESS_NS;
    L.sums = L.tpart + npairs * T * T * 2;
    L.rec = L.sums + HESS_NS + 2 * npairs + q * q;
    L.total = L.rec + 3 + q + q * q;
    return L;
}

}  // namespace

size_t hess_buf_doubles(int n, int n_ell) { return hess_layout(n, n_ell).total; }

double *hess_record(double *buf, int n, int n_ell) { return buf + hess_layout(n, n_ell).rec; }

void launch_hess(const gpmi_ctx *c, hipStream_t s, double *buf, const double *X, int n, int ldx, const SeParams &p, double alpha,
                 const double *ell, int n_ell, double sigma, double diag_add, const double *y, const double *av, double asign,
                 const double *Wk, size_t ld, const double *gsums, int gns, const int *info, double *hess, int ldh)
{
    const int m = n_ell, q = 2 + m, m1 = m + 1, npairs = m1 * (m1 + 1) / 2;
    const HessLayout L = hess_layout(n, m);
    const unsigned T = (unsigned)((n + 63) / 64), nchunk = (unsigned)((n + HESS_CH - 1) / HESS_CH), nb = (unsigned)((n + 255) / 256);
    const size_t ntiles = (size_t)T * (T + 1) / 2;
    double *Sm = buf + L.S, *P = buf + L.P, *Af = buf + L.A, *Bv = buf + L.Bv, *Cv = buf + L.Cv;
    double *hs = buf + L.sums, *ts = hs + HESS_NS, *dots = ts + 2 * npairs;
    // 1. operands: A (full), K o R_d, b
    hipLaunchKernelGGL(k_hess_operands, dim3(T, T), 256, 0, s, X, n, ldx, p, m, av, asign, Wk, ld, Af, Sm, L.ldm, L.mstride, buf + L.bpart);
    hipLaunchKernelGGL(k_hess_bsum, dim3(nb), 256, 0, s, buf + L.bpart, (int)T, n, m, av, asign, y, diag_add, alpha, sigma, Bv);
    // 2. P_d = A (K o R_d) = A (K o R_d)^T on the matrix cores
    for (int d = 0; d < m; ++d)
        launch_gemm_nt(c, s, Af, L.ldm, Sm + (size_t)d * L.mstride, L.ldm, P + (size_t)d * L.mstride, L.ldm, n, n, n, 0);
    // 3. pair traces
    hipLaunchKernelGGL(k_hess_traces, dim3(T, T, (unsigned)npairs), 256, 0, s, P, L.ldm, L.mstride, n, m1, buf + L.tpart);
    hipLaunchKernelGGL(k_hess_sum, dim3((unsigned)npairs), 1024, 0, s, buf + L.tpart, (size_t)T * T * 2, (size_t)T * T, 2, ts);
    // 4. second-order contraction
    if (m == 1) {
        hipLaunchKernelGGL(k_hess_second_iso, dim3(T, T), 256, 0, s, X, n, ldx, p, av, Wk, ld, buf + L.hpart);
        hipLaunchKernelGGL(k_hess_sum, dim3(1), 1024, 0, s, buf + L.hpart, (size_t)0, ntiles, 1, hs);
    } else {
        hipLaunchKernelGGL(k_hess_second_ard, dim3(T, T), 256, 0, s, X, n, ldx, p, av, Wk, ld, buf + L.hpart);
        hipLaunchKernelGGL(k_hess_sum, dim3(1), 1024, 0, s, buf + L.hpart, (size_t)0, ntiles, HESS_NS, hs);
    }
    // 5. c_j = A b_j and the dots b_i' c_j
    hipLaunchKernelGGL(k_hess_mv_part, dim3(nb, nchunk), 256, 0, s, Af, L.ldm, n, Bv, q, buf + L.cpart);
    hipLaunchKernelGGL(k_hess_mv_sum, dim3(nb, (unsigned)q), 256, 0, s, buf + L.cpart, n, (int)nchunk, q, Cv);
    hipLaunchKernelGGL(k_hess_dots, dim3((unsigned)q, (unsigned)q), 256, 0, s, Bv, Cv, n, q, dots);
    // 6. finish
    HessFinish f;
    f.alpha = alpha;
    f.sigma = sigma;
    f.s = diag_add;
    f.e = grad_ell(ell, n_ell);
    f.n = n;
    f.D = p.D;
    f.m = m;
    f.gns = gns;
    hipLaunchKernelGGL(k_hess_finish, dim3(1), 64, 0, s, gsums, hs, ts, dots, f, info, hess, ldh);
}
