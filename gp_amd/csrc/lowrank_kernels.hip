// Low-rank GP from the Hermite eigenfunctions of the squared-exponential kernel (gpmi_hermite_basis, gpmi_lowrank_logml_grad,
// gpmi_lowrank_latent_lp_grad; gfx950 only).  With a = 1 / (4 scale^2), eps^2 = 1 / (2 l^2), alpha^2 = 2 a,
// beta = (1 + 4 eps^2 / alpha^2)^(1/4), delta^2 = alpha^2 (beta^2 - 1) / 2, Dn = alpha^2 + delta^2 + eps^2 and r = eps^2 / Dn,
// column k = 0 .. M - 1 of Phi is
//   psi_k(x) = amp (alpha^2 / Dn)^(1/4) sqrt(beta r^k / (2^k k!)) exp(-delta^2 x^2) H_k(alpha beta x),
// and the columns obey   psi_{k+1} = p_k x psi_k - q_k psi_{k-1},  p_k = alpha beta sqrt(2 r / (k + 1)),  q_k = r sqrt(k / (k + 1)),
// psi_0 = c0 exp(-delta^2 x^2).  lr_row is the ONE statement of that recurrence and of its tangent in l; every kernel here
// generates the basis with it, so Phi has the same bits wherever it is formed and is never stored outside gpmi_hermite_basis.
// Every sum has a fixed shape and order: no atomics, repeated calls give identical bits.
#include "chol_device.h"
#include "latent_device.h"

namespace {

constexpr int LR_MP = GPMI_LR_MMAX;   // pitch of the four coefficient arrays in LDS

// p_k, dp_k / dl, q_k, dq_k / dl for k = threadIdx.x < M: once per workgroup, from the launch's scalars
__device__ __forceinline__ void lr_coef(const LrPar &P, int M, double *cf)
{
    const int k = threadIdx.x;
    if (k < M && k < LR_MP) {
        const double k1 = (double)(k + 1);
        const double p = P.ab * sqrt(2.0 * P.r / k1), s = sqrt((double)k / k1);
        cf[k] = p;
        cf[LR_MP + k] = p * P.pl;
        cf[2 * LR_MP + k] = P.r * s;
        cf[3 * LR_MP + k] = P.dr * s;
    }
}

// The recurrence as a state: lr_first is column 0 at x, lr_next(k) moves from column k to column k + 1
struct LrState {
    double x, v, dv, vm, dvm;   // psi_k, its l-tangent, and those of column k - 1
};
__device__ __forceinline__ LrState lr_first(const LrPar &P, double x)
{
    const double x2 = x * x;
    const double e = exp(-(P.d2 * x2));
    LrState s;
    s.x = x;
    s.v = P.c0 * e;
    s.dv = P.dc0 * e - P.dd2 * x2 * s.v;
    s.vm = s.dvm = 0.0;
    return s;
}
__device__ __forceinline__ void lr_next(const double *cf, LrState &s, int k)
{
    const double p = cf[k], dp = cf[LR_MP + k], q = cf[2 * LR_MP + k], dq = cf[3 * LR_MP + k];
    const double xv = s.x * s.v;
    const double vn = p * xv - q * s.vm;
    const double dvn = (dp * xv + p * (s.x * s.dv)) - (dq * s.vm + q * s.dvm);
    s.vm = s.v;
    s.dvm = s.dv;
    s.v = vn;
    s.dv = dvn;
}
// value and l-tangent of the M columns at x, handed to f(k, psi_k, dpsi_k / dl) in column order
template <class F>
__device__ __forceinline__ void lr_row(const LrPar &P, const double *cf, double x, int M, F &&f)
{
    LrState s = lr_first(P, x);
    f(0, s.v, s.dv);
    for (int k = 0; k + 1 < M; ++k) {
        lr_next(cf, s, k);
        f(k + 1, s.v, s.dv);
    }
}

// Phi (n x M, ldp) and, when dPhi != nullptr, dPhi / dl (lddp): one thread per row, stores along the rows of a column
__global__ __launch_bounds__(256) void k_lr_basis(const double *__restrict__ x, int n, int M, LrPar P, double *__restrict__ Phi, size_t ldp,
                                                  double *__restrict__ dPhi, size_t lddp)
{
    __shared__ double cf[4 * LR_MP];
    lr_coef(P, M, cf);
    __syncthreads();
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)n) return;
    lr_row(P, cf, x[i], M, [&](int k, double v, double dv) {
        Phi[i + (size_t)k * ldp] = v;
        if (dPhi) dPhi[i + (size_t)k * lddp] = dv;
    });
}

// ---- the Gram product ---------------------------------------------------------------------------------------------------
// MT = ceil(M / 16) column tiles.  A workgroup (four waves) owns `rows` consecutive rows and walks them in sub-blocks of RB:
// the first RB threads (all 256 up to M = 32) generate one row each into LDS (column-major, pitch RB + 2: the generating stores run along a column
// and the operand loads of a 16 x 4 fragment touch every bank once), then the waves share the MT (MT + 1) / 2 lower tile pairs
// (i >= j) round-robin and add, with v_mfma_f64_16x16x4_f64, G_ij += Phi_i' Phi_j and S_ij += Phi_i' dPhi_j + dPhi_i' Phi_j,
// while thread t adds its entry of b = Phi' y (t < MP) or c = dPhi' y (MP <= t < 2 MP) and the last thread y'y, rows in order.
// Rows past the chunk's end and columns past M are zeros in LDS.  One partial per chunk:
//   part[chunk * lr_part_doubles(MT)]: per pair p = i (i + 1) / 2 + j the G tile (256, row-major) and the S tile, then b (MP),
//   c (MP), y'y.
template <int MT>
struct LrGram {
    static constexpr int MP = 16 * MT;
    static constexpr int RB = MT <= 2 ? 256 : (MT <= 4 ? 128 : 64);   // 2 MP (RB + 2) doubles of LDS: at most 135 KB of the CU's 160
    static constexpr int RBP = RB + 2;
    static constexpr int T = MT * (MT + 1) / 2;
    static constexpr int NP = (T + 3) / 4;
};

template <int MT>
__global__ __launch_bounds__(256) void k_lr_gram(const double *__restrict__ x, const double *__restrict__ y, int n, int M, LrPar P,
                                                 int rows, double *__restrict__ part, size_t pstride)
{
    using C = LrGram<MT>;
    constexpr int MP = C::MP, RB = C::RB, RBP = C::RBP, T = C::T, NP = C::NP;
    __shared__ double sP[MP * RBP], sD[MP * RBP], sy[RB], cf[4 * LR_MP];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    lr_coef(P, M, cf);
    int ti[NP], tj[NP];
#pragma unroll
    for (int q = 0; q < NP; ++q) {
        const int p = w + 4 * q;
        int i = 0;
        while ((i + 1) * (i + 2) / 2 <= p) ++i;
        ti[q] = i;
        tj[q] = p - i * (i + 1) / 2;
    }
    d4 G[NP], S[NP];
#pragma unroll
    for (int q = 0; q < NP; ++q) G[q] = S[q] = d4{0.0, 0.0, 0.0, 0.0};
    double vacc = 0.0, yacc = 0.0;
    const long long row0 = (long long)blockIdx.x * rows;
    const long long row1 = row0 + rows < (long long)n ? row0 + rows : (long long)n;
    __syncthreads();
    for (long long base = row0; base < row1; base += RB) {
        if (tid < RB) {
            const long long row = base + tid;
            if (row < row1) {
                sy[tid] = y[row];
                lr_row(P, cf, x[row], M, [&](int k, double v, double dv) {
                    sP[k * RBP + tid] = v;
                    sD[k * RBP + tid] = dv;
                });
                for (int k = M; k < MP; ++k) sP[k * RBP + tid] = sD[k * RBP + tid] = 0.0;
            } else {
                sy[tid] = 0.0;
                for (int k = 0; k < MP; ++k) sP[k * RBP + tid] = sD[k * RBP + tid] = 0.0;
            }
        }
        __syncthreads();
        const int co = lane & 15;
        for (int ks = 0; ks < RB / 4; ++ks) {
            const int ro = 4 * ks + (lane >> 4);
#pragma unroll
            for (int q = 0; q < NP; ++q) {
                if (w + 4 * q < T) {
                    const int oi = (16 * ti[q] + co) * RBP + ro, oj = (16 * tj[q] + co) * RBP + ro;
                    const double ai = sP[oi], di = sD[oi], aj = sP[oj], dj = sD[oj];
                    G[q] = mfma(ai, aj, G[q]);
                    S[q] = mfma(ai, dj, S[q]);
                    S[q] = mfma(di, aj, S[q]);
                }
            }
        }
        if (tid < 2 * MP) {
            const double *col = tid < MP ? sP + tid * RBP : sD + (tid - MP) * RBP;
            for (int r = 0; r < RB; ++r) vacc += col[r] * sy[r];
        }
        if (tid == 255)
            for (int r = 0; r < RB; ++r) yacc += sy[r] * sy[r];
        __syncthreads();
    }
    double *out = part + (size_t)blockIdx.x * pstride;
#pragma unroll
    for (int q = 0; q < NP; ++q) {
        const int p = w + 4 * q;
        if (p < T) {
#pragma unroll
            for (int g = 0; g < 4; ++g) {   // row (lane >> 4) + 4 g, column lane & 15 of the tile
                out[(size_t)p * 512 + 64 * g + lane] = G[q][g];
                out[(size_t)p * 512 + 256 + 64 * g + lane] = S[q][g];
            }
        }
    }
    if (tid < 2 * MP) out[(size_t)T * 512 + tid] = vacc;
    if (tid == 255) out[(size_t)T * 512 + 2 * MP] = yacc;
}

// ---- the finishing kernel: ONE workgroup of 1024 threads ------------------------------------------------------------------
// Partials added in chunk order; A = sigma^2 I + G in LDS (column-major, pitch MP + 1) and the full S (in LDS up to MP = 64:
// BIG = false; in `sg`, MP x MP, beyond); left-looking Cholesky of A, one thread per row; W = L^-1 column by column (thread j
// owns column j and stores W(k, j), k > j, at A(j, k): the strict upper triangle; the diagonal follows once L is spent);
// t = W b, u = W' t;
//   T = tr A^-1 = |W|_F^2,  <A^-1, S> = sum_{j <= k} (W S)_kj W_kj, the entries (k, j) dealt round-robin to the threads and the
//   1024 sums added by one tree,
// and the results.  A pivot <= 0 (or NaN) at order k: *info = k, out3 and grad (when given) NaN.
template <bool BIG>
__global__ __launch_bounds__(1024) void k_lr_finish(const double *__restrict__ part, size_t pstride, int nchunks, int n, int M, int MT,
                                                    double amp, double sigma, double *__restrict__ sg, double *__restrict__ out3,
                                                    double *__restrict__ grad, int *__restrict__ info)
{
    constexpr int AM = BIG ? 128 : 64;
    __shared__ double A[AM * (AM + 1)], sS[BIG ? 1 : 64 * 65];
    __shared__ double sb[LR_MP], sc[LR_MP], st[LR_MP], su[LR_MP], winv[LR_MP], csq[LR_MP], slog[LR_MP], red[1024];
    __shared__ double piv, syy;
    const int tid = threadIdx.x, MP = 16 * MT, AP = MP + 1, T = MT * (MT + 1) / 2;
    double *S = BIG ? sg : sS;
    const int SP = BIG ? MP : MP + 1;
    const double s2 = sigma * sigma;
    for (int e = tid; e < M * M; e += 1024) {
        const int R = e % M, Cc = e / M;
        if (R < Cc) continue;
        const int p = (R >> 4) * ((R >> 4) + 1) / 2 + (Cc >> 4);
        const size_t o = (size_t)p * 512 + (size_t)(R & 15) * 16 + (Cc & 15);
        double g = 0.0, s = 0.0;
#pragma unroll 8   // eight chunks' loads in flight; the additions keep chunk order
        for (int c = 0; c < nchunks; ++c) {
            g += part[(size_t)c * pstride + o];
            s += part[(size_t)c * pstride + o + 256];
        }
        A[R + Cc * AP] = R == Cc ? g + s2 : g;
        S[R + Cc * SP] = s;
        S[Cc + R * SP] = s;
    }
    if (tid < 2 * M) {
        const int k = tid < M ? tid : tid - M;
        const size_t o = (size_t)T * 512 + (tid < M ? k : MP + k);
        double a = 0.0;
#pragma unroll 8
        for (int c = 0; c < nchunks; ++c) a += part[(size_t)c * pstride + o];
        (tid < M ? sb : sc)[k] = a;
    }
    if (tid == 1023) {
        double a = 0.0;
#pragma unroll 8
        for (int c = 0; c < nchunks; ++c) a += part[(size_t)c * pstride + (size_t)T * 512 + 2 * MP];
        syy = a;
    }
    __syncthreads();
    // left-looking Cholesky: thread i forms v_i = A(i, k) - sum_{j < k} L(i, j) L(k, j), j ascending
    int fail = 0;
    for (int k = 0; k < M; ++k) {
        double v = 0.0;
        if (tid >= k && tid < M) {
            v = A[tid + k * AP];
#pragma unroll 8
            for (int j = 0; j < k; ++j) v -= A[tid + j * AP] * A[k + j * AP];
            if (tid == k) piv = v;
        }
        __syncthreads();
        const double d = piv;
        if (!(d > 0.0)) {
            fail = k + 1;
            break;
        }
        const double s = sqrt(d);
        if (tid >= k && tid < M) A[tid + k * AP] = tid == k ? s : v / s;
        __syncthreads();
    }
    if (fail) {
        if (tid == 0) {
            const double nan = __builtin_nan("");
            *info = fail;
            out3[0] = out3[1] = out3[2] = nan;
            if (grad) grad[0] = grad[1] = grad[2] = nan;
        }
        return;
    }
    // W = L^-1: thread j, rows in order; the loop bounds are uniform so that L(i, k) is one broadcast load
    if (tid < M) {
        const int j = tid;
        double sq = 0.0, wjj = 0.0;
        for (int i = 0; i < M; ++i) {
            double acc = i == j ? 1.0 : 0.0;
#pragma unroll 8
            for (int k = 0; k < i; ++k)
                if (k >= j) acc -= A[i + k * AP] * (k == j ? wjj : A[j + k * AP]);
            if (i >= j) {
                const double wv = acc / A[i + i * AP];
                if (i == j) wjj = wv;
                else A[j + i * AP] = wv;
                sq += wv * wv;
            }
        }
        winv[j] = wjj;
        csq[j] = sq;
        slog[j] = log(A[j + j * AP]);
    }
    __syncthreads();
    if (tid < M) A[tid + tid * AP] = winv[tid];   // L is spent: row k of W is now A(0 .. k, k)
    __syncthreads();
    if (tid < M) {   // t = W b
        double a = 0.0;
        for (int j = 0; j <= tid; ++j) a += A[j + tid * AP] * sb[j];
        st[tid] = a;
    }
    __syncthreads();
    if (tid < M) {   // u = W' t
        double a = 0.0;
        for (int i = tid; i < M; ++i) a += A[tid + i * AP] * st[i];
        su[tid] = a;
    }
    __syncthreads();
    {   // (W S)_kj W_kj, j <= k: k runs along the threads (W's rows sit at the odd pitch AP, S(i, j) is one broadcast load)
        double a = 0.0;
        for (int e = tid; e < M * M; e += 1024) {
            const int k = e % M, j = e / M;
            if (j > k) continue;
            double r = 0.0;
#pragma unroll 8
            for (int i = 0; i <= k; ++i) r += A[i + k * AP] * S[i + j * SP];
            a += r * A[j + k * AP];
        }
        red[tid] = a;
    }
    __syncthreads();
    for (int h = 512; h > 0; h >>= 1) {
        if (tid < h) red[tid] += red[tid + h];
        __syncthreads();
    }
    if (tid == 0) {
        double tt = 0.0, uu = 0.0, uc = 0.0, T1 = 0.0, ld = 0.0;
        for (int k = 0; k < M; ++k) {
            tt += st[k] * st[k];
            uu += su[k] * su[k];
            uc += su[k] * sc[k];
            T1 += csq[k];
            ld += slog[k];
        }
        sb[0] = tt;   // b is spent
        sb[1] = uu;
        sb[2] = uc;
        sb[3] = T1;
        sb[4] = ld;
    }
    __syncthreads();
    const double trs = red[0], tt = sb[0], uu = sb[1], uc = sb[2], T1 = sb[3], ld = sb[4];
    __syncthreads();
    if (tid < M) {   // u' S u
        double r = 0.0;
        for (int j = 0; j < M; ++j) r += S[tid + j * SP] * su[j];
        red[tid] = su[tid] * r;
    }
    __syncthreads();
    if (tid == 0) {
        double usu = 0.0;
        for (int k = 0; k < M; ++k) usu += red[k];
        const double nm = (double)n - (double)M, Md = (double)M;
        const double Q = (syy - tt) / s2;
        const double hld = nm * log(sigma) + ld;
        *info = 0;
        out3[0] = -hld - 0.5 * Q - 0.91893853320467274178 * (double)n;
        out3[1] = hld;
        out3[2] = Q;
        if (grad) {
            grad[0] = (uu - Md + s2 * T1) / amp;
            grad[1] = (uc - 0.5 * usu) / s2 - 0.5 * trs;
            grad[2] = Q / sigma - uu / sigma - nm / sigma - sigma * T1;
        }
    }
}

// ---- the latent form ------------------------------------------------------------------------------------------------------
// A workgroup owns 256 rows.  Pass 1, thread = row: q = Phi z and qd = dPhi z from the recurrence (columns in order), the head,
// qbar; the four row terms (lik, d lik / d sigma, qbar q, qbar qd) by one tree over the workgroup.  Pass 2 regenerates the
// recurrence and reduces psi_k qbar over the rows, 16 columns at a time through LDS: 16 interleaved runs of 16 rows, then the 16
// runs in order.  One workgroup (n <= 256) writes the results itself; otherwise its 4 + M partials go to part[blockIdx.x * (4 + M)]
// and k_lr_latent_sum adds them in workgroup order.
constexpr int LR_ZP = 257;

__global__ __launch_bounds__(256) void k_lr_latent(const double *__restrict__ x, int n, int M, LrPar P, double amp, const double *__restrict__ z,
                                                   LatentHead lh, double *__restrict__ q, double *__restrict__ qbar,
                                                   double *__restrict__ part, double *__restrict__ out, double *__restrict__ zbar,
                                                   double *__restrict__ grad)
{
    __shared__ double cf[4 * LR_MP], sz[LR_MP], buf[16 * LR_ZP], ps[16 * 16], red[4][256];
    const int tid = threadIdx.x;
    lr_coef(P, M, cf);
    if (tid < M) sz[tid] = z[tid];
    __syncthreads();
    const size_t i = (size_t)blockIdx.x * 256 + tid;
    const bool live = i < (size_t)n;
    const double xi = live ? x[i] : 0.0;
    double qb = 0.0;
    {
        double qv = 0.0, qd = 0.0, lik = 0.0, dsig = 0.0, fb1;
        if (live) {
            lr_row(P, cf, xi, M, [&](int k, double v, double dv) {
                qv += v * sz[k];
                qd += dv * sz[k];
            });
            latent_head_row(lh, qv, 0.0, lh.Y + i, lik, dsig, qb, fb1);
            if (q) q[i] = qv;
            if (qbar) qbar[i] = qb;
        }
        red[0][tid] = lik;
        red[1][tid] = dsig;
        red[2][tid] = qb * qv;
        red[3][tid] = qb * qd;
    }
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (tid < h)
            for (int a = 0; a < 4; ++a) red[a][tid] += red[a][tid + h];
        __syncthreads();
    }
    const bool single = gridDim.x == 1;
    double *po = part + (size_t)blockIdx.x * (4 + M);
    if (tid == 0) {
        if (single) {
            out[0] = red[0][0];
            out[1] = red[1][0];
            grad[0] = red[2][0] / amp;
            grad[1] = red[3][0];
        } else {
            for (int a = 0; a < 4; ++a) po[a] = red[a][0];
        }
    }
    LrState rs = lr_first(P, xi);
    for (int k0 = 0; k0 < M; k0 += 16) {
        for (int k = k0; k < k0 + 16; ++k) {   // columns past M and rows past n: zeros
            if (k > 0 && k < M) lr_next(cf, rs, k - 1);
            buf[(k - k0) * LR_ZP + tid] = live && k < M ? rs.v * qb : 0.0;
        }
        __syncthreads();
        {
            const int k = tid >> 4, seg = tid & 15;
            double a = 0.0;
            for (int r = 0; r < 16; ++r) a += buf[k * LR_ZP + r * 16 + seg];
            ps[k * 16 + seg] = a;
        }
        __syncthreads();
        if (tid < 16 && k0 + tid < M) {
            double a = 0.0;
            for (int s = 0; s < 16; ++s) a += ps[tid * 16 + s];
            if (single) zbar[k0 + tid] = a;
            else po[4 + k0 + tid] = a;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void k_lr_latent_sum(const double *__restrict__ part, int nwg, int M, double amp, double *__restrict__ out,
                                                       double *__restrict__ zbar, double *__restrict__ grad)
{
    const int t = threadIdx.x;
    if (t >= 4 + M) return;
    double a = 0.0;
    for (int g = 0; g < nwg; ++g) a += part[(size_t)g * (4 + M) + t];
    if (t == 0) out[0] = a;
    else if (t == 1) out[1] = a;
    else if (t == 2) grad[0] = a / amp;
    else if (t == 3) grad[1] = a;
    else zbar[t - 4] = a;
}

}  // namespace

LrPar lr_params(double scale, double amp, double l)
{
    // alpha^2 is fixed by scale; everything else moves with l.  delta^2 = alpha^2 (beta^2 - 1) / 2 = 2 eps^2 / (beta^2 + 1): the
    // second form has no cancellation when l is large against scale
    const double al2 = 1.0 / (2.0 * scale * scale), al = sqrt(al2);
    const double ep2 = 1.0 / (2.0 * l * l), dep2 = -1.0 / (l * l * l);
    const double be = sqrt(sqrt(1.0 + 4.0 * ep2 / al2));
    const double dbe = dep2 / (al2 * be * be * be);
    const double d2 = 2.0 * ep2 / (be * be + 1.0), dd2 = al2 * be * dbe;
    const double Dn = al2 + d2 + ep2, dDn = dd2 + dep2;
    LrPar P;
    P.r = ep2 / Dn;
    P.dr = (dep2 * Dn - ep2 * dDn) / (Dn * Dn);
    P.c0 = amp * sqrt(sqrt(al2 / Dn)) * sqrt(be);
    P.dc0 = P.c0 * (0.5 * dbe / be - 0.25 * dDn / Dn);
    P.d2 = d2;
    P.dd2 = dd2;
    P.ab = al * be;
    P.pl = dbe / be + 0.5 * P.dr / P.r;
    return P;
}

void launch_lr_basis(hipStream_t s, const double *x, int n, int M, const LrPar &P, double *Phi, size_t ldp, double *dPhi, size_t lddp)
{
    hipLaunchKernelGGL(k_lr_basis, dim3((n + 255) / 256), 256, 0, s, x, n, M, P, Phi, ldp, dPhi, lddp);
}

// rows per chunk and number of chunks: a function of (n, M) alone.  Whole sub-blocks (RB rows: 256 up to M = 32, 128 up to 64,
// 64 beyond) and at most 256 chunks (one per compute unit): the finishing kernel reads every partial once
int lr_gram_rows(int n, int M)
{
    const int MT = (M + 15) / 16, RB = MT <= 2 ? 256 : (MT <= 4 ? 128 : 64);
    const long long per = ((long long)n + 255) / 256;          // rows per chunk for 256 chunks
    return (int)(((per + RB - 1) / RB) * RB);
}
int lr_gram_chunks(int n, int M) { return (n + lr_gram_rows(n, M) - 1) / lr_gram_rows(n, M); }
size_t lr_part_doubles(int M)
{
    const size_t MT = (size_t)(M + 15) / 16;
    return MT * (MT + 1) / 2 * 512 + 2 * 16 * MT + 8;
}
size_t lr_scratch_doubles(int n, int M)
{
    const size_t MP = (size_t)(M + 15) / 16 * 16;
    return (size_t)lr_gram_chunks(n, M) * lr_part_doubles(M) + MP * MP;
}

template <int MT>
static void lr_gram_mt(hipStream_t s, const double *x, const double *y, int n, int M, const LrPar &P, double *part)
{
    hipLaunchKernelGGL(k_lr_gram<MT>, dim3(lr_gram_chunks(n, M)), 256, 0, s, x, y, n, M, P, lr_gram_rows(n, M), part, lr_part_doubles(M));
}

void launch_lr_logml(hipStream_t s, const double *x, int n, const double *y, int M, const LrPar &P, double amp, double sigma,
                     double *scratch, double *out3, double *grad, int *info)
{
    const int MT = (M + 15) / 16, MP = 16 * MT, nch = lr_gram_chunks(n, M);
    switch (MT) {
    case 1: lr_gram_mt<1>(s, x, y, n, M, P, scratch); break;
    case 2: lr_gram_mt<2>(s, x, y, n, M, P, scratch); break;
    case 3: lr_gram_mt<3>(s, x, y, n, M, P, scratch); break;
    case 4: lr_gram_mt<4>(s, x, y, n, M, P, scratch); break;
    case 5: lr_gram_mt<5>(s, x, y, n, M, P, scratch); break;
    case 6: lr_gram_mt<6>(s, x, y, n, M, P, scratch); break;
    case 7: lr_gram_mt<7>(s, x, y, n, M, P, scratch); break;
    default: lr_gram_mt<8>(s, x, y, n, M, P, scratch); break;
    }
    double *sg = scratch + (size_t)nch * lr_part_doubles(M);
    if (MP <= 64)
        hipLaunchKernelGGL(k_lr_finish<false>, dim3(1), 1024, 0, s, scratch, lr_part_doubles(M), nch, n, M, MT, amp, sigma, sg, out3, grad, info);
    else
        hipLaunchKernelGGL(k_lr_finish<true>, dim3(1), 1024, 0, s, scratch, lr_part_doubles(M), nch, n, M, MT, amp, sigma, sg, out3, grad, info);
}

int lr_latent_blocks(int n) { return (n + 255) / 256; }

void launch_lr_latent(hipStream_t s, const double *x, int n, int M, const LrPar &P, double amp, const double *z, const LatentHead &lh,
                      double *q, double *qbar, double *part, double *out, double *zbar, double *grad)
{
    const int nwg = lr_latent_blocks(n);
    hipLaunchKernelGGL(k_lr_latent, dim3(nwg), 256, 0, s, x, n, M, P, amp, z, lh, q, qbar, part, out, zbar, grad);
    if (nwg > 1) hipLaunchKernelGGL(k_lr_latent_sum, dim3(1), 256, 0, s, part, nwg, M, amp, out, zbar, grad);
}
