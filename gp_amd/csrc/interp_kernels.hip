// Reverse mode of the interpolated latent-GP transforms (models/cubic_interpolated_gp.hpp:6-32,38-73 and
// models/interpolated_gp.stan:9-47): one pass over T stored lower triangles M_t (column-major, ld x n each) with value
// weights a_t and tangent weights b_t, A = sum a_t M_t, B = sum b_t M_t:
//   F = A Z (nullable),  Zbar = A^T Fbar,  lbar = sum_c Fbar[:,c]^T (B Z[:,c]).
// Every table element is read once per call (k <= 8 columns per pass) and blended once; the blended value feeds the row
// sums (F, B Z) and the column sums (Zbar).  Memory-bound: T n(n+1)/2 doubles per pass.
//
// Layout of the pass: a workgroup (256 threads, thread = row) owns 256 rows x one 128-column chunk, as k_hermite_mv does.
// Row sums are chunk partials in ascending j; chunk totals are added in ascending chunk order (for the Hermite blend the
// additions of k_hermite_mv_small / k_hermite_mv + k_hermite_mv_sum: F is bit-identical to gpmi_approx_Lz).  Column sums
// are reduced over each wave by a fixed xor butterfly, the four wave sums of a workgroup in wave order, and the row blocks
// in ascending order by a second small launch (k_tri_vjp_fin).  No atomics, no counters: results do not depend on
// scheduling.  n <= 256 and k <= 8: one launch of one workgroup (k_tri_vjp_small), inputs possibly host-mapped.
#include "gpmi_internal.h"

namespace {
#include "interp_device.h"

constexpr int TV_ROWS = 256;  // rows of a workgroup (one per thread)
constexpr int TV_CW = 128;    // columns of a chunk (== HMV_CW of se_kernels.hip)
constexpr int TV_KG = GPMI_TRI_KG;

// the cubic Hermite blend of the interval's four triangles: a = v(l), b = dv/dl (cubic_interpolated_gp.hpp:62-67), the
// operation order of k_hermite_mv
struct HermiteSrc {
    const double *L1, *L2, *D1, *D2;
    size_t ld;
    double dx, t, dtdl;

    __device__ __forceinline__ void prologue(double *) const {}

    template <int G>
    __device__ __forceinline__ void blend(const double *, int i, int jb, int jlast, double (&a)[G], double (&b)[G]) const
    {
        double y1[G], y2[G], k1[G], k2[G];
#pragma unroll
        for (int q = 0; q < G; ++q) {
            const int j = jb + q < jlast ? jb + q : jlast;
            const size_t o = (size_t)i + (size_t)j * ld;
            y1[q] = L1[o];
            y2[q] = L2[o];
            k1[q] = D1[o];
            k2[q] = D2[o];
        }
#pragma unroll
        for (int q = 0; q < G; ++q) {
            a[q] = hermite(y1[q], y2[q], k1[q], k2[q], dx, t);
            const double aa = k1[q] * dx - (y2[q] - y1[q]);
            const double bb = -k2[q] * dx + (y2[q] - y1[q]);
            b[q] = (bb * (2 - 3 * t) * t + aa * (1 + t * (-4 + 3 * t)) - y1[q] + y2[q]) * dtdl;
        }
    }
};

// weights of the GP-regression lookup (interpolated_gp.stan:40-41 with length-scale rho):
// w_p = exp(-(l - lp_p)^2 / (2 rho^2)), w'_p = -(l - lp_p) / rho^2 w_p
__device__ __forceinline__ void gp_weights(const double *lp, int P, double l, double rho, double *sw)
{
    for (int p = threadIdx.x; p < P; p += blockDim.x) {
        const double d = l - lp[p];
        const double w = exp(-(d * d) / (2 * rho * rho));
        sw[p] = w;
        sw[GPMI_GP_PMAX + p] = -d / (rho * rho) * w;
    }
}

// the GP-regression blend: a = sum_p w_p M_p[i,j], b = sum_p w'_p M_p[i,j], ascending p (weights in LDS)
struct GpSrc {
    const double *M;
    size_t ld, msz;
    int P;
    const double *lp;
    double l, rho;

    __device__ __forceinline__ void prologue(double *sw) const { gp_weights(lp, P, l, rho, sw); }

    template <int G>
    __device__ __forceinline__ void blend(const double *sw, int i, int jb, int jlast, double (&a)[G], double (&b)[G]) const
    {
#pragma unroll
        for (int q = 0; q < G; ++q) a[q] = b[q] = 0.0;
        size_t o[G];
#pragma unroll
        for (int q = 0; q < G; ++q) o[q] = (size_t)i + (size_t)(jb + q < jlast ? jb + q : jlast) * ld;
        for (int p0 = 0; p0 < P; p0 += 4) {
            double m[4][G];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const size_t base = (size_t)(p0 + u < P ? p0 + u : P - 1) * msz;
#pragma unroll
                for (int q = 0; q < G; ++q) m[u][q] = M[base + o[q]];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (p0 + u < P) {
                    const double w = sw[p0 + u], wd = sw[GPMI_GP_PMAX + p0 + u];
#pragma unroll
                    for (int q = 0; q < G; ++q) {
                        a[q] += w * m[u][q];
                        b[q] += wd * m[u][q];
                    }
                }
            }
        }
    }
};

__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);  // a + b == b + a: every lane ends with the same bits
    return v;
}

// sum over the 256 threads of a workgroup, fixed tree; red: 256 doubles of LDS; result valid in every thread
__device__ __forceinline__ double block_sum(double v, double *red)
{
    red[threadIdx.x] = v;
    __syncthreads();
    for (int s = TV_ROWS / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}

// One 256-row x 128-column block of the pass.  szc: Z of the chunk in LDS ([col - j0][KM]); s_zb: [4 waves][TV_CW][KM]
// LDS wave sums of the column products (written for every column of the chunk); af / ag: the row's chunk partials of
// A Z and B Z (ascending j).
template <int KM, int G, class Src>
__device__ __forceinline__ void tri_block(const Src &src, const double *sw, int n, int rb, int ch, int kk, bool vjp,
                                          const double *szc, double *s_zb, const double (&fb)[KM], double (&af)[KM],
                                          double (&ag)[KM])
{
    static_assert(TV_CW % G == 0, "column groups tile the chunk");
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int i = rb * TV_ROWS + tid;
    const int il = i < n ? i : n - 1;  // rows past n load row n - 1 and contribute nothing
    const int j0 = ch * TV_CW;
    const int jend = j0 + TV_CW < n ? j0 + TV_CW : n;
    const int wlast = rb * TV_ROWS + wv * 64 + 63 < n - 1 ? rb * TV_ROWS + wv * 64 + 63 : n - 1;
    const int jw = jend < wlast + 1 ? jend : wlast + 1;  // columns this wave has entries in (wave-uniform)
#pragma unroll
    for (int c = 0; c < KM; ++c) af[c] = ag[c] = 0.0;
    for (int jb = j0; jb < jend; jb += G) {
        if (jb < jw) {
            double a[G], b[G];
            src.template blend<G>(sw, il, jb, jend - 1, a, b);
            bool on[G];
#pragma unroll
            for (int q = 0; q < G; ++q) on[q] = (jb + q <= i) && (i < n) && (jb + q < jend);
#pragma unroll
            for (int q = 0; q < G; ++q) {
                if (on[q]) {
#pragma unroll
                    for (int c = 0; c < KM; ++c) {
                        if (c < kk) {
                            af[c] += a[q] * szc[(jb + q - j0) * KM + c];
                            ag[c] += b[q] * szc[(jb + q - j0) * KM + c];
                        }
                    }
                }
            }
            if (vjp) {
                double v[G][KM];
#pragma unroll
                for (int q = 0; q < G; ++q)
#pragma unroll
                    for (int c = 0; c < KM; ++c) v[q][c] = (on[q] && c < kk) ? a[q] * fb[c] : 0.0;
#pragma unroll
                for (int q = 0; q < G; ++q)
#pragma unroll
                    for (int c = 0; c < KM; ++c) v[q][c] = wave_sum(v[q][c]);
                if (lane == 0) {
#pragma unroll
                    for (int q = 0; q < G; ++q)
#pragma unroll
                        for (int c = 0; c < KM; ++c) s_zb[(wv * TV_CW + jb + q - j0) * KM + c] = v[q][c];
                }
            }
        } else if (vjp && lane == 0) {
#pragma unroll
            for (int q = 0; q < G; ++q)
#pragma unroll
                for (int c = 0; c < KM; ++c) s_zb[(wv * TV_CW + jb + q - j0) * KM + c] = 0.0;
        }
    }
}

// the four wave sums of column j (chunk-local jl), wave order
template <int KM>
__device__ __forceinline__ double wave_partials(const double *s_zb, int jl, int c)
{
    return ((s_zb[(0 * TV_CW + jl) * KM + c] + s_zb[(1 * TV_CW + jl) * KM + c]) + s_zb[(2 * TV_CW + jl) * KM + c]) +
           s_zb[(3 * TV_CW + jl) * KM + c];
}

// n <= 256, k <= KM: the whole pass in one workgroup.  Z, Fb, F, Zb, lbar may be host-mapped (each read or written once).
// LDS: Z [n][KM] | wave sums [4][TV_CW][KM] | reduction [256] | weights [2 GPMI_GP_PMAX]
template <int KM, int G, class Src>
__global__ __launch_bounds__(256) void k_tri_vjp_small(Src src, int n, const double *__restrict__ Z, int ldz,
                                                       const double *__restrict__ Fb, int ldfb, int kk,
                                                       double *__restrict__ F, int ldf, double *__restrict__ Zb, int ldzb,
                                                       double *__restrict__ lbar)
{
    extern __shared__ double sm[];
    double *sz = sm;
    double *s_zb = sz + (size_t)n * KM;
    double *red = s_zb + 4 * TV_CW * KM;
    double *sw = red + TV_ROWS;
    const bool vjp = Fb != nullptr;
    for (int e = threadIdx.x; e < n * KM; e += TV_ROWS) {
        const int j = e / KM, c = e % KM;
        sz[e] = c < kk ? Z[(size_t)j + (size_t)c * ldz] : 0.0;
    }
    src.prologue(sw);
    __syncthreads();
    const int i = threadIdx.x;
    double fb[KM], tf[KM], tg[KM];
#pragma unroll
    for (int c = 0; c < KM; ++c) {
        fb[c] = (vjp && i < n && c < kk) ? Fb[(size_t)i + (size_t)c * ldfb] : 0.0;
        tf[c] = tg[c] = 0.0;
    }
    const int nch = (n + TV_CW - 1) / TV_CW;
    for (int ch = 0; ch < nch; ++ch) {
        double af[KM], ag[KM];
        tri_block<KM, G>(src, sw, n, 0, ch, kk, vjp, sz + (size_t)ch * TV_CW * KM, s_zb, fb, af, ag);
#pragma unroll
        for (int c = 0; c < KM; ++c) {
            tf[c] += af[c];
            tg[c] += ag[c];
        }
        __syncthreads();
        if (vjp) {
            for (int e = threadIdx.x; e < TV_CW * KM; e += TV_ROWS) {
                const int jl = e / KM, c = e % KM, j = ch * TV_CW + jl;
                if (j < n && c < kk) {
                    double acc = 0.0;
                    acc += wave_partials<KM>(s_zb, jl, c);
                    Zb[(size_t)j + (size_t)c * ldzb] = acc;
                }
            }
        }
        __syncthreads();
    }
    if (F && i < n) {
#pragma unroll
        for (int c = 0; c < KM; ++c)
            if (c < kk) F[(size_t)i + (size_t)c * ldf] = tf[c];
    }
    if (vjp) {
        double lr = 0.0;
#pragma unroll
        for (int c = 0; c < KM; ++c)
            if (c < kk) lr += fb[c] * tg[c];
        const double s = block_sum(i < n ? lr : 0.0, red);
        if (threadIdx.x == 0) *lbar = s;
    }
}

// any n: workgroup (row block rb = blockIdx.x, chunk ch = blockIdx.y); chunks right of the block's diagonal do nothing.
// part_f / part_g: [chunk][c][row] row partials; part_zb: [row block][c][col] column partials (vjp only)
template <int KM, int G, class Src>
__global__ __launch_bounds__(256) void k_tri_vjp(Src src, int n, const double *__restrict__ Z, int ldz,
                                                 const double *__restrict__ Fb, int ldfb, int kk, double *__restrict__ part_f,
                                                 double *__restrict__ part_g, double *__restrict__ part_zb)
{
    const int rb = blockIdx.x, ch = blockIdx.y;
    if (ch * TV_CW > rb * TV_ROWS + TV_ROWS - 1) return;
    __shared__ double sz[TV_CW * KM];
    __shared__ double s_zb[4 * TV_CW * KM];
    __shared__ double sw[2 * GPMI_GP_PMAX];
    const bool vjp = Fb != nullptr;
    const int j0 = ch * TV_CW;
    for (int e = threadIdx.x; e < TV_CW * KM; e += TV_ROWS) {
        const int j = j0 + e / KM, c = e % KM;
        sz[e] = (c < kk && j < n) ? Z[(size_t)j + (size_t)c * ldz] : 0.0;
    }
    src.prologue(sw);
    __syncthreads();
    const int i = rb * TV_ROWS + threadIdx.x;
    double fb[KM], af[KM], ag[KM];
#pragma unroll
    for (int c = 0; c < KM; ++c) fb[c] = (vjp && i < n && c < kk) ? Fb[(size_t)i + (size_t)c * ldfb] : 0.0;
    tri_block<KM, G>(src, sw, n, rb, ch, kk, vjp, sz, s_zb, fb, af, ag);
    if (i < n) {
#pragma unroll
        for (int c = 0; c < KM; ++c) {
            if (c < kk) {
                part_f[((size_t)ch * kk + c) * n + i] = af[c];
                if (vjp) part_g[((size_t)ch * kk + c) * n + i] = ag[c];
            }
        }
    }
    if (vjp) {
        __syncthreads();
        for (int e = threadIdx.x; e < TV_CW * KM; e += TV_ROWS) {
            const int jl = e / KM, c = e % KM, j = j0 + jl;
            if (j < n && c < kk) part_zb[((size_t)rb * kk + c) * n + j] = wave_partials<KM>(s_zb, jl, c);
        }
    }
}

// thread t: row t (F, and lrow[t] = sum_c Fbar[t,c] (B Z)[t,c]) and column t (Zbar); every sum in a fixed order
__global__ __launch_bounds__(256) void k_tri_vjp_fin(int n, int kk, int nrb, const double *__restrict__ part_f,
                                                     const double *__restrict__ part_g, const double *__restrict__ part_zb,
                                                     const double *__restrict__ Fb, int ldfb, double *__restrict__ F, int ldf,
                                                     double *__restrict__ Zb, int ldzb, double *__restrict__ lrow)
{
    const int t = blockIdx.x * TV_ROWS + threadIdx.x;
    if (t >= n) return;
    const int cmax = t / TV_CW;  // chunks right of the diagonal hold nothing for this row
    double lr = 0.0;
    for (int c = 0; c < kk; ++c) {
        double f = 0.0;
        for (int ch = 0; ch <= cmax; ++ch) f += part_f[((size_t)ch * kk + c) * n + t];
        if (F) F[(size_t)t + (size_t)c * ldf] = f;
        if (Fb) {
            double g = 0.0;
            for (int ch = 0; ch <= cmax; ++ch) g += part_g[((size_t)ch * kk + c) * n + t];
            lr += Fb[(size_t)t + (size_t)c * ldfb] * g;
        }
    }
    if (!Fb) return;
    lrow[t] = lr;
    for (int c = 0; c < kk; ++c) {
        double acc = 0.0;
        for (int rb = t / TV_ROWS; rb < nrb; ++rb) acc += part_zb[((size_t)rb * kk + c) * n + t];  // row blocks with rows >= t
        Zb[(size_t)t + (size_t)c * ldzb] = acc;
    }
}

// lbar = sum over column groups and rows of lrow, fixed order (one workgroup)
__global__ __launch_bounds__(256) void k_tri_vjp_lsum(const double *__restrict__ lrow, int n, int ng, double *__restrict__ lbar)
{
    __shared__ double red[TV_ROWS];
    double s = 0.0;
    for (int g = 0; g < ng; ++g)
        for (int i = threadIdx.x; i < n; i += TV_ROWS) s += lrow[(size_t)g * n + i];
    s = block_sum(s, red);
    if (threadIdx.x == 0) *lbar = s;
}

// L(l) = sum_p w_p M_p (lower triangle, zero above): thread = row, 16 columns per workgroup
__global__ __launch_bounds__(256) void k_gp_blend(GpSrc src, int n, double *__restrict__ out, size_t ldo)
{
    __shared__ double sw[2 * GPMI_GP_PMAX];
    src.prologue(sw);
    __syncthreads();
    const int i = blockIdx.x * TV_ROWS + threadIdx.x;
    if (i >= n) return;
    for (int j = blockIdx.y * 16; j < n && j < (int)blockIdx.y * 16 + 16; ++j) {
        double a = 0.0;
        if (j <= i) {
            const size_t o = (size_t)i + (size_t)j * src.ld;
            for (int p = 0; p < src.P; ++p) a += sw[p] * src.M[(size_t)p * src.msz + o];
        }
        out[(size_t)i + (size_t)j * ldo] = a;
    }
}

// lookup = (Sigma_P \ exact)^T (interpolated_gp.stan:10-27), in place: entry (i, j) of the P stacked triangles is the
// right-hand side e_p = M_p[i, j]; x = U^-1 L^-1 (perm e) by forward and back substitution with the partial-pivot LU
// factors of Sigma_P (row-major P x P, unit lower L below the diagonal) in LDS; M_p[i, j] = x_p.  One entry per thread,
// its P values in an LDS column of its own ([p][64]); entries above the diagonal are set to zero.  64 threads x 64 columns
// per workgroup.  LDS: (P^2 + 64 P) doubles <= 64 KiB.
__global__ __launch_bounds__(64) void k_gp_lookup(double *__restrict__ M, size_t ld, size_t msz, int n, int P,
                                                  const double *__restrict__ lu, const int *__restrict__ perm)
{
    extern __shared__ double sm[];
    double *slu = sm;
    double *sv = sm + (size_t)P * P;
    const int tid = threadIdx.x;
    const int i = blockIdx.x * 64 + tid;
    const int jb = blockIdx.y * 64;
    const int jmax = jb + 64 < n ? jb + 64 : n;
    if (jb > (int)blockIdx.x * 64 + 63) {  // tile above the diagonal
        if (i < n)
            for (int j = jb; j < jmax; ++j)
                for (int p = 0; p < P; ++p) M[(size_t)p * msz + (size_t)i + (size_t)j * ld] = 0.0;
        return;
    }
    for (int e = tid; e < P * P; e += 64) slu[e] = lu[e];
    __syncthreads();
    if (i >= n) return;
    for (int j = jb; j < jmax; ++j) {
        const size_t o = (size_t)i + (size_t)j * ld;
        if (j > i) {
            for (int p = 0; p < P; ++p) M[(size_t)p * msz + o] = 0.0;
            continue;
        }
        for (int p = 0; p < P; ++p) {  // L y = perm e
            double y = M[(size_t)perm[p] * msz + o];
            for (int q = 0; q < p; ++q) y -= slu[p * P + q] * sv[q * 64 + tid];
            sv[p * 64 + tid] = y;
        }
        for (int p = P - 1; p >= 0; --p) {  // U x = y
            double x = sv[p * 64 + tid];
            for (int q = p + 1; q < P; ++q) x -= slu[p * P + q] * sv[q * 64 + tid];
            sv[p * 64 + tid] = x / slu[p * P + p];
        }
        for (int p = 0; p < P; ++p) M[(size_t)p * msz + o] = sv[p * 64 + tid];
    }
}

template <int KM, int G, class Src>
void tri_pass(hipStream_t s, const Src &src, int n, const double *Z, int ldz, const double *Fb, int ldfb, int kk, double *F,
              int ldf, double *Zb, int ldzb, double *lbar, double *ws, int g, int ng, bool one)
{
    if (one) {
        const size_t lds = ((size_t)n * KM + 4 * TV_CW * KM + TV_ROWS + 2 * GPMI_GP_PMAX) * sizeof(double);
        hipLaunchKernelGGL((k_tri_vjp_small<KM, G, Src>), dim3(1), dim3(TV_ROWS), lds, s, src, n, Z, ldz, Fb, ldfb, kk, F, ldf,
                           Zb, ldzb, lbar);
        return;
    }
    const int nrb = (n + TV_ROWS - 1) / TV_ROWS, nch = (n + TV_CW - 1) / TV_CW;
    double *part_f = ws, *part_g = part_f + (size_t)nch * TV_KG * n, *part_zb = part_g + (size_t)nch * TV_KG * n;
    double *lrow = part_zb + (size_t)nrb * TV_KG * n;
    hipLaunchKernelGGL((k_tri_vjp<KM, G, Src>), dim3(nrb, nch), dim3(TV_ROWS), 0, s, src, n, Z, ldz, Fb, ldfb, kk, part_f,
                       part_g, part_zb);
    hipLaunchKernelGGL(k_tri_vjp_fin, dim3(nrb), dim3(TV_ROWS), 0, s, n, kk, nrb, part_f, part_g, part_zb, Fb, ldfb, F, ldf,
                       Zb, ldzb, lrow + (size_t)g * n);
    if (Fb && g == ng - 1) hipLaunchKernelGGL(k_tri_vjp_lsum, dim3(1), dim3(TV_ROWS), 0, s, lrow, n, ng, lbar);
}

template <class Src>
void tri_vjp(hipStream_t s, const Src &src, int n, const double *Z, int ldz, const double *Fb, int ldfb, int k, double *F,
             int ldf, double *Zb, int ldzb, double *lbar, double *ws)
{
    const bool one = tri_vjp_one_launch(n, k);
    const int ng = (k + TV_KG - 1) / TV_KG;
    for (int g = 0; g < ng; ++g) {
        const int c0 = g * TV_KG, kk = k - c0 < TV_KG ? k - c0 : TV_KG;
        const double *Zg = Z + (size_t)c0 * ldz;
        const double *Fbg = Fb ? Fb + (size_t)c0 * ldfb : nullptr;
        double *Fg = F ? F + (size_t)c0 * ldf : nullptr;
        double *Zbg = Zb ? Zb + (size_t)c0 * ldzb : nullptr;
        if (kk == 1)
            tri_pass<1, 8>(s, src, n, Zg, ldz, Fbg, ldfb, kk, Fg, ldf, Zbg, ldzb, lbar, ws, g, ng, one);
        else
            tri_pass<TV_KG, 2>(s, src, n, Zg, ldz, Fbg, ldfb, kk, Fg, ldf, Zbg, ldzb, lbar, ws, g, ng, one);
    }
}
}  // namespace

bool tri_vjp_one_launch(int n, int k) { return n <= GPMI_TRI_SMALL_N && k <= TV_KG; }

size_t tri_vjp_ws_doubles(int n, int k)
{
    const size_t nrb = (n + TV_ROWS - 1) / TV_ROWS, nch = (n + TV_CW - 1) / TV_CW, ng = (k + TV_KG - 1) / TV_KG;
    return (2 * nch + nrb) * TV_KG * (size_t)n + ng * (size_t)n;
}

void launch_hermite_vjp(hipStream_t s, const double *L1, const double *L2, const double *D1, const double *D2, size_t ld, int n,
                        double x1, double x2, double l, const double *Z, int ldz, const double *Fb, int ldfb, int k, double *F,
                        int ldf, double *Zb, int ldzb, double *lbar, double *ws)
{
    if (n <= 0 || k <= 0) return;
    // t, dx and dt/dl as launch_hermite_mv forms them
    const double t = (l - x1) / (x2 - x1);
    const double dtdl = 1 / (x2 - x1);
    const HermiteSrc src{L1, L2, D1, D2, ld, x2 - x1, t, dtdl};
    tri_vjp(s, src, n, Z, ldz, Fb, ldfb, k, F, ldf, Zb, ldzb, lbar, ws);
}

void launch_gp_vjp(hipStream_t s, const double *M, size_t ld, int n, int P, const double *lp, double rho, double l,
                   const double *Z, int ldz, const double *Fb, int ldfb, int k, double *F, int ldf, double *Zb, int ldzb,
                   double *lbar, double *ws)
{
    if (n <= 0 || k <= 0) return;
    const GpSrc src{M, ld, ld * (size_t)n, P, lp, l, rho};
    tri_vjp(s, src, n, Z, ldz, Fb, ldfb, k, F, ldf, Zb, ldzb, lbar, ws);
}

void launch_gp_blend(hipStream_t s, const double *M, size_t ld, int n, int P, const double *lp, double rho, double l,
                     double *out, size_t ldo)
{
    if (n <= 0) return;
    const GpSrc src{M, ld, ld * (size_t)n, P, lp, l, rho};
    hipLaunchKernelGGL(k_gp_blend, dim3((n + TV_ROWS - 1) / TV_ROWS, (n + 15) / 16), dim3(TV_ROWS), 0, s, src, n, out, ldo);
}

void launch_gp_lookup(hipStream_t s, double *M, size_t ld, int n, int P, const double *lu, const int *perm)
{
    if (n <= 0) return;
    const size_t lds = ((size_t)P * P + 64 * (size_t)P) * sizeof(double);
    hipLaunchKernelGGL(k_gp_lookup, dim3((n + 63) / 64, (n + 63) / 64), dim3(64), lds, s, M, ld, ld * (size_t)n, n, P, lu, perm);
}
