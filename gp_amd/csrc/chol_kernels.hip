// Blocked right-looking fp64 Cholesky for gfx950 built on v_mfma_f64_16x16x4_f64.
//
// Everything is expressed in 16x16 tiles held in the MFMA accumulator layout
//   D[i][j]: lane l holds i = (l>>4) + 4*reg, j = l&15       (reg = 0..3)
// whose register `reg` is, lane for lane, also a valid A operand
// (A[i=l&15][k=(l>>4)+4*kg]) of the transposed tile and a valid B operand
// (B[k=(l>>4)+4*kg][j=l&15]) of the tile itself.  A tile therefore feeds the
// next MFMA straight from registers: no LDS round trip, no shuffles.
//
// We always compute the TRANSPOSE of the mathematical block, D[n][m] with m the
// matrix row: for column-major storage a register then covers 16 consecutive
// rows (128 contiguous bytes) of 4 columns.
//
// Kernels
//   k_potrf_diag4 one workgroup: factor a <=128x128 diagonal block, emit its
//                 factors packed in fragment order (Fpack) for the panel solve
//   k_trsm_panel  rows below the block: X = A21 L11^-T by blocked substitution,
//                 each wave owns 16 rows and chains MFMAs through registers
//   k_gemm_nt     C -= A B^T / C = A B^T, 128x128 tiles, LDS-staged with
//                 global_load_lds, 2-stage pipeline; SYRK mode walks only the
//                 lower-triangular tiles of the trailing matrix
// The device functions behind these kernels (potrf_diag4_body, trsm_panel_body, gemm_tile, gemm_quad64) live in
// chol_device.h: the one-workgroup kernels of small_kernels.hip inline them too.  This file keeps the blocked kernels,
// the triangular helpers (k_trsv_wave, k_trmv_*, k_logml_partial / finalize, k_get_row, k_pack_factors, ...), the
// probe build's instruments, gpmi_tuning_defaults and the panel scheduler.  The tile walks of the SYRK mode (syrk_tile,
// syrk_tile_bands) and the launch plan of the trailing update (syrk_plan) are host-and-device integer code in syrk_walk.h.
// Reference: Stan cholesky_decompose (models/fit_hyperparameters.stan:25),
// multi_normal_cholesky (:31), L*z (models/exact_gp.stan:25).
#include "chol_device.h"

namespace {

__global__ __launch_bounds__(256, 2) void k_potrf_diag4(double *__restrict__ A, size_t lda, int nb_act,
                                                     double *__restrict__ Fpack, int *info, int col0)
{
    __shared__ double sm[DIAG4_LDS];
    if (nb_act == GPMI_NB) potrf_diag4_body<false, true>(sm, A, lda, nb_act, Fpack, info, col0);
    else potrf_diag4_body<false, false>(sm, A, lda, nb_act, Fpack, info, col0);
}

__global__ __launch_bounds__(256) void k_trsm_panel(double *__restrict__ Acol, size_t lda, int row0,
                                                    int M, int nb_act, const double *__restrict__ Fpack)
{
    __shared__ __attribute__((aligned(16))) double s_F[GPMI_FPACK];
    {
        const double2 *src = reinterpret_cast<const double2 *>(Fpack);
        double2 *dst = reinterpret_cast<double2 *>(s_F);
#pragma unroll
        for (int q = 0; q < GPMI_FPACK / 2 / 256; ++q) dst[threadIdx.x + 256 * q] = src[threadIdx.x + 256 * q];
    }
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int rbase = row0 + blockIdx.x * 64;
    const int r = rbase + w * 16 + (lane & 15);
    if (nb_act == GPMI_NB && rbase + 64 <= M)  // workgroup-uniform
        trsm_panel_body<true>(s_F, Acol, lda, r, true, nb_act);
    else
        trsm_panel_body<false>(s_F, Acol, lda, r, r < M, nb_act);
}

// Two workgroups share a CU and its matrix pipes.  All tiles cost the same, so workgroups that
// start together stay in lock-step: both reach their memory-bound epilogue at the same time
// and the pipes idle.  Delaying the second-dispatched workgroup of each CU once, by about one
// epilogue, puts the pair in anti-phase for the rest of the launch: one streams its C tile
// while the other has the pipes to itself.
// stagger = (mode << 16) | sleeps; mode 1: blocks 256..511 (second dispatch round),
// mode 2: odd hardware wave slot of wave 0 (HW_REG_HW_ID[3:0]).
__device__ __forceinline__ void stagger_start(double (&smem)[2][2][GK][GP], int stagger)
{
    if ((stagger & 0xffffff) && blockIdx.x < 512) {
        bool late = false;
        if (((stagger >> 16) & 0xff) == 1) late = blockIdx.x >= 256;
        else {
            if (threadIdx.x == 0) smem[0][0][0][0] = (double)(__builtin_amdgcn_s_getreg((31 << 11) | 4) & 1);
            __syncthreads();
            late = smem[0][0][0][0] != 0.0;
            __syncthreads();
        }
        if (late)
            for (int i = 0; i < (stagger & 0xffff); ++i) __builtin_amdgcn_s_sleep(127);
    }
}

// Fused look-ahead: the workgroup of tile (0, 0) -- the 128 x 128 diagonal block of the NEXT panel
// whenever the update starts at the row of its first column -- factors that block as soon as its
// own tile is stored, while the other workgroups of the launch are still updating.  The
// diagonal-block latency chain (27 us per panel) then runs inside the update instead of after
// it, needs no launch and no free CU of its own, and the panel solve follows directly.
struct FuseDiag {
    double *Fp;   // packed-factor slot of that panel; nullptr: no fusion
    int *info;
    int col0;     // global column of the block (for info)
    int nb;       // active order of the block (<= 128)
    int *ctr;     // zeroed device counter for the sub-tiled variant (order bit 9)
};

// 16 x 16 sub-tile of C -= A B^T at (m0, n0), ONE wave, fragments straight from global memory with EVERY
// load of a 128-wide K range in flight at once (two sets of 16 k-groups = 64 loads per lane): the operands
// were written by the previous kernel on other CUs / XCDs and come from HBM or the Infinity Cache, so
// the cost of a sub-tile is memory round trips, not matrix work -- the 64 x 64 form above (8 k-groups in
// flight behind 8 being multiplied) took 3 dependent round trips at K = 128 (~11 us), this one takes one.
// Two accumulators halve the dependent MFMA chain.  Requires K % 64 == 0; the tile lies wholly inside C.
template <bool COH = false>
__device__ __forceinline__ void gemm_sub16(const double *__restrict__ A, size_t lda, const double *__restrict__ B, size_t ldb,
                                           double *__restrict__ C, size_t ldc, int K, int m0, int n0)
{
    const int lane = threadIdx.x & 63;
    const int lr = lane & 15, lq = lane >> 4;
    const double *pa = A + (size_t)(m0 + lr) + (size_t)lq * lda;  // bf = pa[k * lda]
    const double *pb = B + (size_t)(n0 + lr) + (size_t)lq * ldb;  // af = pb[k * ldb]
    d4 acc0 = d4{0.0, 0.0, 0.0, 0.0}, acc1 = acc0;
    double fa[2][16], fb[2][16];
    // ONE running offset per operand, opaque to the optimiser: with per-load offsets it materialises all 64
    // addresses (128 registers) next to the 128 registers of loaded operands and spills the operands (the
    // offset, not the pointer, is made opaque: the loads stay global_load, not flat_load)
    const size_t sa = 4 * lda, sb = 4 * ldb;
    auto load = [&](int set, int k0) {
        size_t oa = (size_t)k0 * lda, ob = (size_t)k0 * ldb;
#pragma unroll
        for (int g = 0; g < 16; ++g) {
            fa[set][g] = pb[ob];
            fb[set][g] = pa[oa];
            oa += sa;
            ob += sb;
            asm volatile("" : "+v"(oa), "+v"(ob));
        }
    };
    auto mul = [&](int set) {
#pragma unroll
        for (int g = 0; g < 16; g += 2) {
            acc0 = mfma(fa[set][g], fb[set][g], acc0);
            acc1 = mfma(fa[set][g + 1], fb[set][g + 1], acc1);
        }
    };
    load(0, 0);
    if (K > 64) load(1, 64);
#pragma unroll 1
    for (int k0 = 0; k0 < K; k0 += 128) {
        mul(0);
        if (k0 + 128 < K) load(0, k0 + 128);
        if (k0 + 64 < K) {
            mul(1);
            if (k0 + 192 < K) load(1, k0 + 192);
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        double *q = C + (size_t)(m0 + lr) + (size_t)(n0 + lq + 4 * i) * ldc;
        const double v = *q - (acc0[i] + acc1[i]);
        if constexpr (COH) __hip_atomic_store(q, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        else *q = v;
    }
}

#ifdef GPMI_PROBES
// shader-clock probe: per workgroup of the SYRK kernel, elapsed shader cycles (s_memtime) and elapsed
// 100 MHz reference ticks (s_memrealtime), summed over the launch -> average clock and cycles per tile
__device__ unsigned long long g_clk[4];
__device__ unsigned long long g_fz[8];  // fused in-block launch, block 0: cycles in sub-tile, flag wait, diagonal body; launches
#endif

// Blocks 0 .. SUBWG - 1 of a sub-tiled fused launch (order bit 9): the 36 lower 16 x 16 sub-tiles of the
// diagonal tile (0, 0), one per wave; block 0 then waits for the other eight on fd.ctr and factors the block.
// The SUBWG blocks are the first of the grid -- dispatched together, so the wait cannot deadlock.
__device__ __forceinline__ void fused_subtiles_and_diag(double (&smem)[2][2][GK][GP], int b, const double *__restrict__ A, size_t lda,
                                                        const double *__restrict__ B, size_t ldb, double *__restrict__ C, size_t ldc,
                                                        int K, const FuseDiag &fd)
{
#ifdef GPMI_PROBES
    const unsigned long long fz0 = __builtin_amdgcn_s_memtime();
#endif
    {
        const int t = b * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // sub-tile index, row-major lower triangle
        int tm = 0;
        while ((tm + 1) * (tm + 2) / 2 <= t) ++tm;
        const int tn = t - tm * (tm + 1) / 2;
        gemm_sub16<true>(A, lda, B, ldb, C, ldc, K, tm * 16, tn * 16);
    }
    // the agent-scope stores above are complete (acknowledged by the memory side) once
    // vmcnt drains; no cache-wide fence is needed around this hand-over
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (b) {
        if (threadIdx.x == 0) atomicAdd(fd.ctr, 1);
        return;
    }
#ifdef GPMI_PROBES
    const unsigned long long fz1 = __builtin_amdgcn_s_memtime();
#endif
    if (threadIdx.x == 0) {
        while (__hip_atomic_load(fd.ctr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < SUBWG - 1)
            __builtin_amdgcn_s_sleep(4);
        __hip_atomic_store(fd.ctr, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // next launch is stream-ordered
    }
    __syncthreads();
#ifdef GPMI_PROBES
    const unsigned long long fz2 = __builtin_amdgcn_s_memtime();
#endif
    if (fd.nb == GPMI_NB) potrf_diag4_body<true, true>(&smem[0][0][0][0], C, ldc, fd.nb, fd.Fp, fd.info, fd.col0);
    else potrf_diag4_body<true, false>(&smem[0][0][0][0], C, ldc, fd.nb, fd.Fp, fd.info, fd.col0);
#ifdef GPMI_PROBES
    if (threadIdx.x == 0) {
        atomicAdd(&g_fz[0], fz1 - fz0);
        atomicAdd(&g_fz[1], fz2 - fz1);
        atomicAdd(&g_fz[2], __builtin_amdgcn_s_memtime() - fz2);
        atomicAdd(&g_fz[3], 1ull);
        atomicAdd(&g_fz[4], (unsigned long long)K);
        if (K == 128) {  // leaf launches: the body IS the critical path there
            atomicAdd(&g_fz[5], __builtin_amdgcn_s_memtime() - fz2);
            atomicAdd(&g_fz[6], fz1 - fz0);
            atomicAdd(&g_fz[7], 1ull);
        }
    }
#endif
}

template <int MODE>
__global__ __launch_bounds__(256, 2) void k_gemm_nt(const double *__restrict__ A, size_t lda,
                                                 const double *__restrict__ B, size_t ldb,
                                                 double *__restrict__ C, size_t ldc, int M, int N, int K, int order,
                                                 int stagger, FuseDiag fd, KSplit ks)
{
    static_assert(2 * 2 * GK * GP >= DIAG4_LDS, "the diagonal-block body runs in the staging buffer");
    __shared__ __attribute__((aligned(16))) double smem[2][2][GK][GP];
    // bits 24+ of `stagger` are probe-only switches (tools/syrk_bench.py): 1 = skip the C
    // epilogue, 2 = skip the operand streaming of the main loop; used for the cost breakdown
    // in DESIGN.md.  They exist in the probe build only; here they fold to nothing.
#ifdef GPMI_PROBES
    const int dbg = stagger >> 24;
    struct ClkProbe {
        unsigned long long t0, r0;
        __device__ ClkProbe() : t0(__builtin_amdgcn_s_memtime()), r0(__builtin_amdgcn_s_memrealtime()) {}
        __device__ ~ClkProbe()
        {
            if (MODE == 1 && threadIdx.x == 0) {
                atomicAdd(&g_clk[0], __builtin_amdgcn_s_memtime() - t0);
                atomicAdd(&g_clk[1], __builtin_amdgcn_s_memrealtime() - r0);
                atomicAdd(&g_clk[2], 1ull);
            }
        }
    } clk_probe;
#else
    constexpr int dbg = 0;
#endif
    stagger_start(smem, stagger);
    int ti, tj;
    if (MODE == 1) {
        int b = blockIdx.x;
        if (order & 0x200) {  // sub-tiled fused launch: tile 0 = the next diagonal block, by the first SUBWG blocks
            if (b < SUBWG) {
                fused_subtiles_and_diag(smem, b, A, lda, B, ldb, C, ldc, K, fd);
                return;
            }
            b -= SUBWG - 1;   // blocks SUBWG, ... are the tiles 1, 2, ...
        }
        const int T = (M + GT - 1) / GT;
        const int TN = (N + GT - 1) / GT < T ? (N + GT - 1) / GT : T;
        if ((order & 0xff) == 2) {  // XCD-partitioned band walk (multi-round launches)
            const int nt = TN * (TN + 1) / 2 + (T - TN) * TN;
            const int S = (nt + 7) >> 3;
            int c, quad = -1;  // quad < 0: the whole tile
            if (b < 8 * S) {
                const int s = b >> 3;
                c = (b & 7) * S + s;
                if (ks.S > 1 && s >= ks.bfull) quad = 0;  // last partial round of this XCD: quadrant 0 here, 1 .. 3 behind the grid
            } else {
                const int e = b - 8 * S, Rx = S - ks.bfull, t = e / 3;
                quad = 1 + e - 3 * t;
                c = (t / Rx) * S + ks.bfull + t % Rx;
            }
            if (c >= nt) return;
            syrk_tile_bands(c, T, TN, ti, tj);
            const bool thin = ti == T - 1 && T > 1 && M - ti * GT <= 64 && K % GK == 0;  // e.g. the augmented row alone
            if (quad >= 0 || thin) {
                for (int q = quad >= 0 ? quad : 0; q < (quad >= 0 ? quad + 1 : 4); ++q) {
                    const int qm = q & 1, qn = (q >> 1) & 1;
                    const int m0 = ti * GT + qm * 64, n0 = tj * GT + qn * 64;
                    if ((ti == tj && qn > qm) || m0 >= M || n0 >= N) continue;  // workgroup-uniform
                    gemm_quad64(&smem[0][0][0][0], A + m0, lda, B + n0, ldb, C + (size_t)m0 + (size_t)n0 * ldc, ldc, K, M - m0,
                                N - n0, (int)threadIdx.x);
                    __syncthreads();
                }
                return;
            }
        } else
        if (ks.S > 1 && b >= ks.bfull) {
            const int q = b - ks.bfull;
            if (!syrk_tile(ks.bfull + (q >> 2), T, TN, order & 0xff, ti, tj)) return;
            const int qm = q & 1, qn = (q >> 1) & 1;
            if (ti == tj && qn > qm) return;  // strictly upper quadrant of a diagonal tile
            const int m0 = ti * GT + qm * 64, n0 = tj * GT + qn * 64;
            if (m0 >= M || n0 >= N) return;
            gemm_quad64(&smem[0][0][0][0], A + m0, lda, B + n0, ldb, C + (size_t)m0 + (size_t)n0 * ldc, ldc, K, M - m0,
                        N - n0, (int)threadIdx.x);
            return;
        }
        if ((order & 0xff) != 2 && !syrk_tile(b, T, TN, order & 0xff, ti, tj)) return;
        // order bit 8: the panel is UPPER TRIANGULAR (P[i][k] = 0 for k < i, e.g. L^-T): the
        // products of tile (ti, tj), tj <= ti, start at column ti * 128 -- a third of the work of
        // the full update; row-major tile order runs the long tiles first
        if (order & 0x100) {
            const int k0 = ti * GT;
            A += (size_t)k0 * lda;
            B += (size_t)k0 * ldb;
            K -= k0;
        }
    } else if (MODE == 0 && (order & 0x200)) {
        // Sub-tiled fused launch (1-D grid): the diagonal tile (0, 0) sits on the critical path of
        // the panel chain and one workgroup needs K * 256 cycles for it, plus the memory latency of
        // operands the previous kernel has just written elsewhere.  Its lower triangle is cut into 36
        // 16 x 16 sub-tiles, one per wave of the first SUBWG = 9 workgroups (dispatched first, so
        // all are resident and the wait below cannot deadlock), each with all its operand loads in
        // flight at once; block 0 waits for the other eight and factors the block.  Blocks >= SUBWG
        // are the tiles 1, 2, ...
        const int b = blockIdx.x;
        if (b < SUBWG) {
            fused_subtiles_and_diag(smem, b, A, lda, B, ldb, C, ldc, K, fd);
            return;
        }
        const int gx = (M + GT - 1) / GT;
        ti = (b - (SUBWG - 1)) % gx;
        tj = (b - (SUBWG - 1)) / gx;
    } else if (MODE == 2 && (order & 0x400)) {
        // C = A B^T for a LOWER-triangular A (M x K, A[i][k] = 0 for k > i) and an UPPER-triangular B (N x K stored
        // with the n index contiguous, B[j][k] = 0 for k < j -- the transpose of a lower-triangular factor): the
        // product is lower triangular, only the tiles ti >= tj are computed (1-D grid, row-major lower triangle) and
        // tile (ti, tj) needs the columns [128 tj, 128 (ti + 1)) only -- a sixth of the full product's work
        if (!syrk_tile(blockIdx.x, (M + GT - 1) / GT, (M + GT - 1) / GT, 0, ti, tj)) return;
        const int k0 = tj * GT, k1 = (ti + 1) * GT < K ? (ti + 1) * GT : K;
        A += (size_t)k0 * lda;
        B += (size_t)k0 * ldb;
        K = k1 - k0;
    } else {
        ti = blockIdx.x;
        tj = blockIdx.y;
        if (MODE == 0 && (order & 0x100)) {  // longest tiles (small ti) first: grid is (tj, ti)
            ti = blockIdx.y;
            tj = blockIdx.x;
        }
        // order bit 8 (plain grid): A is upper-trapezoidal -- A[i][k] = 0 for i > k + koff, koff =
        // fd.col0 (the global column of A's first column; fd carries no fusion here) -- so the
        // products of row-tile ti start at its first non-zero column (X L^-T with triangular X)
        if (MODE == 0 && (order & 0x100)) {
            const int k0 = ti * GT - fd.col0;
            if (k0 > 0) {
                if (k0 >= K) return;
                A += (size_t)k0 * lda;
                B += (size_t)k0 * ldb;
                K -= k0;
            }
        }
    }
    gemm_tile<MODE, MODE == 0 || MODE == 1>(smem, A, lda, B, ldb, C, ldc, M, N, K, ti, tj, dbg, (int)threadIdx.x);  // the updates: pair-row layout
    if (MODE != 2 && fd.Fp && !(order & 0x200) && ti == 0 && tj == 0) {  // workgroup-uniform
        // the tile's stores must be visible to the other waves of this workgroup, which read the
        // block back in the diagonal kernel's register layout
        __threadfence();
        __syncthreads();
        __threadfence();
        if (fd.nb == GPMI_NB) potrf_diag4_body<false, true>(&smem[0][0][0][0], C, ldc, fd.nb, fd.Fp, fd.info, fd.col0);
        else potrf_diag4_body<false, false>(&smem[0][0][0][0], C, ldc, fd.nb, fd.Fp, fd.info, fd.col0);
    }
}

// Packed factors (Fpack) of an ALREADY factored diagonal block: -L tiles in fragment
// order and the inverse of every 16x16 diagonal tile.  Used by solves against a given L.
__global__ __launch_bounds__(512) void k_pack_factors(const double *__restrict__ L11, size_t ldl,
                                                      int nb_act, double *__restrict__ Fpack)
{
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lr = lane & 15, lq = lane >> 4;
    const int row = w * 16 + lr;
#pragma unroll
    for (int kb = 0; kb < 8; ++kb) {
        if (kb < w) {
#pragma unroll
            for (int kg = 0; kg < 4; ++kg) {
                const int col = kb * 16 + lq + 4 * kg;
                const double v = (row < nb_act && col < nb_act) ? L11[(size_t)row + (size_t)col * ldl] : 0.0;
                Fpack[(size_t)(w * (w - 1) / 2 + kb) * 256 + kg * 64 + lane] = -v;
            }
        }
    }
    double rw[16];
#pragma unroll
    for (int c = 0; c < 16; ++c) {
        const int col = w * 16 + c;
        rw[c] = (c <= lr && row < nb_act) ? L11[(size_t)row + (size_t)col * ldl] : ((c == lr) ? 1.0 : 0.0);
    }
    double x[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        double s = (r == lr) ? 1.0 : 0.0;
#pragma unroll
        for (int k = 0; k < r; ++k) s = fma(-readlane64(rw[k], r), x[k], s);
        x[r] = s / readlane64(rw[r], r);
    }
    if (lq == 0) {
#pragma unroll
        for (int j = 0; j < 16; ++j)
            Fpack[(size_t)fp_inv(w) * 256 + (lr >> 2) * 64 + j + 16 * (lr & 3)] = x[j];
    }
}

// ---------------------------------------------------------------------------
// One right-hand side against a given factor: t = L^-1 k (forward substitution), the whitened kernel row of
// the sequential sampler and mdivide_left_tri_low.  The factor is read ONCE (4 n^2 bytes: HBM-bound); what is
// sequential is the chain of the n / 128 diagonal blocks.  Done through the panel kernels a one-row solve is
// 2 n / 128 dependent launches (4.2 ms at n = 16384); here it is ONE launch:
//   workgroup w owns the 128 unknowns of block-row w.  For j = 0 .. w - 1 it takes the 128 x 128 block
//   L[w, j] -- its loads are issued BEFORE it waits for t_j -- multiplies it with t_j as soon as workgroup j
//   has published it, and after j = w - 1 applies the inverse of its diagonal block (k_diag_inv_t) to
//   k_w - sum_j L[w, j] t_j and publishes t_w.
// Publication needs no flag: the output vector is pre-filled with an all-ones bit pattern (a NaN no
// arithmetic produces: a computed NaN is stored as the canonical quiet NaN), every consumer thread polls ITS
// element with agent-scope loads until it is no longer the pattern, and 64-bit agent-scope stores are
// single-copy atomic.  Block-rows are handed out by a device ticket in START order, so a workgroup waits only for
// workgroups that are already running: the waits cannot deadlock, whatever the dispatch order or residency.
// Sums in a fixed order: deterministic.
// ---------------------------------------------------------------------------
constexpr int TSV = 128;
constexpr unsigned long long TSV_EMPTY = ~0ull;

// Dinv[w]: the inverse of the w-th 128 x 128 diagonal block of L, column-major with leading dimension 128
// (element (r, c) at r + 128 c; zero above the diagonal; identity rows / columns past the matrix order).
// From X = I solved against the block by the panel kernel (X L^-T = L^-T), transposed.
__global__ __launch_bounds__(256) void k_eye_blocks(double *__restrict__ X, int nblk)
{
    const int w = blockIdx.x;
    for (int e = threadIdx.x; e < TSV * TSV; e += 256) X[(size_t)w * TSV * TSV + e] = ((e & (TSV - 1)) == (e >> 7)) ? 1.0 : 0.0;
}
__global__ __launch_bounds__(256) void k_transpose_blocks(const double *__restrict__ X, double *__restrict__ D)
{
    __shared__ double t[16][17];
    const size_t base = (size_t)blockIdx.x * TSV * TSV;
    const int bi = (blockIdx.y & 7) * 16, bj = (blockIdx.y >> 3) * 16;
    const int a = threadIdx.x & 15, b = threadIdx.x >> 4;
    t[b][a] = X[base + (bi + a) + (size_t)(bj + b) * TSV];
    __syncthreads();
    D[base + (bj + a) + (size_t)(bi + b) * TSV] = t[a][b];
}

__global__ __launch_bounds__(256) void k_trsv_wave(const double *__restrict__ L, size_t ldl, int n,
                                                   const double *__restrict__ k, double *__restrict__ t,
                                                   const double *__restrict__ Dinv, int *__restrict__ ticket)
{
    __shared__ double ts[TSV];
    __shared__ double red[2][TSV];
    __shared__ int s_w;
    // Block-row by TICKET, not by blockIdx: HIP promises no dispatch order (each XCD deals its share of the grid
    // independently), so "lower blockIdx started earlier" is not a guarantee.  A workgroup that draws ticket w waits
    // only for tickets < w -- workgroups that have already STARTED, are resident and make progress -- whatever the
    // dispatch order and whatever else shares the chip.  The workgroup drawing the last ticket re-arms the counter
    // (the next launch is stream-ordered behind this one).
    if (threadIdx.x == 0) {
        s_w = atomicAdd(ticket, 1);
        if (s_w == (int)gridDim.x - 1) __hip_atomic_store(ticket, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    const int w = s_w, tid = threadIdx.x, r = tid & (TSV - 1), h = tid >> 7;
    const int row = w * TSV + r;
    const bool rok = row < n;
    const size_t rowc = (size_t)(rok ? row : n - 1);
    // this thread's 64 entries of row r of the inverse diagonal block (columns 64 h ...)
    double Dr[64];
    {
        const double *d = Dinv + (size_t)w * TSV * TSV + r + (size_t)(64 * h) * TSV;
#pragma unroll
        for (int q = 0; q < 64; ++q) Dr[q] = d[(size_t)q * TSV];
    }
    const double kv = rok ? k[row] : 0.0;
    double acc = 0.0;
#pragma unroll 1
    for (int j = 0; j < w; ++j) {
        double Lr[64];
        const double *p = L + rowc + (size_t)(j * TSV + 64 * h) * ldl;
#pragma unroll
        for (int q = 0; q < 64; ++q) Lr[q] = p[(size_t)q * ldl];
        if (tid < TSV) {
            const unsigned long long *src = reinterpret_cast<const unsigned long long *>(t) + (size_t)j * TSV + tid;
            unsigned long long u;
            while ((u = __hip_atomic_load(src, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) == TSV_EMPTY) __builtin_amdgcn_s_sleep(1);
            ts[tid] = __longlong_as_double((long long)u);
        }
        __syncthreads();
        double a0 = 0.0, a1 = 0.0;
#pragma unroll
        for (int q = 0; q < 64; q += 2) {
            a0 = fma(Lr[q], ts[64 * h + q], a0);
            a1 = fma(Lr[q + 1], ts[64 * h + q + 1], a1);
        }
        acc += a0 + a1;
        __syncthreads();  // ts is rewritten in the next round
    }
    red[h][r] = acc;
    __syncthreads();
    if (h == 0) ts[r] = rok ? kv - (red[0][r] + red[1][r]) : 0.0;
    __syncthreads();
    double a0 = 0.0, a1 = 0.0;
#pragma unroll
    for (int q = 0; q < 64; q += 2) {  // lower triangle only: a NaN further down the right-hand side stays there
        if (64 * h + q <= r) a0 = fma(Dr[q], ts[64 * h + q], a0);
        if (64 * h + q + 1 <= r) a1 = fma(Dr[q + 1], ts[64 * h + q + 1], a1);
    }
    __syncthreads();
    red[h][r] = a0 + a1;
    __syncthreads();
    if (h == 0 && rok) {
        double v = red[0][r] + red[1][r];
        if (v != v) v = __longlong_as_double(0x7ff8000000000000ll);  // never the "not yet" pattern
        __hip_atomic_store(t + row, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// out[j] = scale * W[row, col0 + j]
__global__ void k_get_row(const double *__restrict__ W, size_t ld, int row, int col0, int m, double scale,
                          double *__restrict__ out)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j < m) out[j] = scale * W[(size_t)row + (size_t)(col0 + j) * ld];
}

// sum log L_ii, z'z (z = row zrow of the factor), logml.  Two launches with a fixed shape (the sums do
// not depend on timing): FIN_WG workgroups reduce 256-element slices of the diagonal -- every L_ii
// sits in a cache line of its own, so the loads want many waves in flight; one workgroup doing all of
// them took 60 us at N = 16384 -- and a last workgroup adds the slice sums in slice order.
__global__ __launch_bounds__(FIN_SLICE) void k_logml_partial(const double *__restrict__ W, size_t ld, int n, int zrow,
                                                             double *__restrict__ part)
{
    __shared__ double s_a[FIN_SLICE], s_b[FIN_SLICE];
    const int i = blockIdx.x * FIN_SLICE + threadIdx.x;
    double a = 0.0, b = 0.0;
    if (i < n) {
        a = log(W[(size_t)i * (ld + 1)]);
        const double z = W[(size_t)zrow + (size_t)i * ld];
        b = z * z;
    }
    s_a[threadIdx.x] = a;
    s_b[threadIdx.x] = b;
    __syncthreads();
    for (int s = FIN_SLICE / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
            s_a[threadIdx.x] += s_a[threadIdx.x + s];
            s_b[threadIdx.x] += s_b[threadIdx.x + s];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        part[2 * blockIdx.x] = s_a[0];
        part[2 * blockIdx.x + 1] = s_b[0];
    }
}

__global__ __launch_bounds__(256) void k_logml_finalize(const double *__restrict__ part, int nslice, int n,
                                                        const int *d_info, double *__restrict__ out3, int *info_out)
{
    __shared__ double s_a[256], s_b[256];
    double a = 0.0, b = 0.0;
    for (int i = threadIdx.x; i < nslice; i += 256) {
        a += part[2 * i];
        b += part[2 * i + 1];
    }
    s_a[threadIdx.x] = a;
    s_b[threadIdx.x] = b;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
            s_a[threadIdx.x] += s_a[threadIdx.x + s];
            s_b[threadIdx.x] += s_b[threadIdx.x + s];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const int info = *d_info;
        if (info_out) *info_out = info;
        if (info) {
            out3[0] = out3[1] = out3[2] = __builtin_nan("");
        } else {
            out3[1] = s_a[0];
            out3[2] = s_b[0];
            out3[0] = -0.5 * s_b[0] - s_a[0] - 0.5 * (double)n * 1.8378770664093454835606594728112;  // log(2 pi)
        }
    }
}

// f = L z, one thread per row (rows coalesced across lanes)
// 512-column chunks on a 2-D grid (a one-thread-per-row loop over all columns is a latency chain at
// large n), chunks wholly above the diagonal skipped, partial sums added in chunk order
constexpr int TMV_COLS = 512;
__global__ __launch_bounds__(256) void k_trmv_lower_part(const double *__restrict__ L, size_t ldl, int n,
                                                         const double *__restrict__ z, double *__restrict__ part)
{
    const int r0 = blockIdx.x * 256, i = r0 + threadIdx.x;
    const int c0 = blockIdx.y * TMV_COLS;
    if (i >= n) return;
    double s = 0.0;
    if (c0 <= r0 + 255) {
        const int c1 = (c0 + TMV_COLS - 1 < i) ? c0 + TMV_COLS - 1 : i;  // last column of this chunk for row i
        for (int k = c0; k <= c1; ++k) s = fma(L[(size_t)i + (size_t)k * ldl], z[k], s);
    }
    part[(size_t)blockIdx.y * n + i] = s;
}

__global__ __launch_bounds__(256) void k_trmv_lower_sum(const double *__restrict__ part, int n, int nchunk,
                                                        double *__restrict__ f)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double s = 0.0;
    for (int q = 0; q < nchunk; ++q) s += part[(size_t)q * n + i];
    f[i] = s;
}

// w = L^T u (column c of u / w: blockIdx.y): one wave per column of L, w_j = sum_{i >= j} L_ij u_i -- the column is
// contiguous, lanes stride its rows with two accumulators, then a fixed butterfly: the order of every addition depends on
// (n, j) only, repeated calls are bit-identical
__global__ __launch_bounds__(256) void k_trmv_lower_t(const double *__restrict__ L, size_t ldl, int n, const double *__restrict__ u,
                                                      size_t ldu, double *__restrict__ w, size_t ldw)
{
    const int j = blockIdx.x * 4 + (int)(threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (j >= n) return;  // wave-uniform
    const double *col = L + (size_t)j * ldl, *uc = u + (size_t)blockIdx.y * ldu;
    double a0 = 0.0, a1 = 0.0;
    int i = j + lane;
    for (; i + 64 < n; i += 128) {
        a0 = fma(col[i], uc[i], a0);
        a1 = fma(col[i + 64], uc[i + 64], a1);
    }
    if (i < n) a0 = fma(col[i], uc[i], a0);
    double v = a0 + a1;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    if (lane == 0) w[(size_t)blockIdx.y * ldw + j] = v;
}

#ifdef GPMI_PROBES
// D = A(16x4) * B(4x16) with the library's operand conventions (layout probe)
__global__ void k_probe_mfma(const double *A, const double *B, double *D)
{
    const int l = threadIdx.x;
    d4 acc = d4{0.0, 0.0, 0.0, 0.0};
    acc = mfma(A[(l & 15) * 4 + (l >> 4)], B[(l >> 4) * 16 + (l & 15)], acc);
#pragma unroll
    for (int i = 0; i < 4; ++i) D[((l >> 4) + 4 * i) * 16 + (l & 15)] = acc[i];
}

__global__ __launch_bounds__(256) void k_probe_peak(double *sink, int iters)
{
    const int l = threadIdx.x;
    d4 c0 = d4{0, 0, 0, 0}, c1 = c0, c2 = c0, c3 = c0, c4 = c0, c5 = c0, c6 = c0, c7 = c0;
    double a = 1.0 + 1e-9 * l, b = 1.0 - 1e-9 * l;
    const unsigned long long t0 = __builtin_amdgcn_s_memtime(), r0 = __builtin_amdgcn_s_memrealtime();
    // inline asm keeps the eight accumulators pinned in VGPRs (the builtin form makes hipcc
    // shuffle them through AGPRs every iteration, which is not what we want to time)
#define GPMI_MFMA_ASM(cc) asm volatile("v_mfma_f64_16x16x4_f64 %0, %1, %2, %0" : "+v"(cc) : "v"(a), "v"(b))
    for (int it = 0; it < iters; ++it) {
        GPMI_MFMA_ASM(c0); GPMI_MFMA_ASM(c1); GPMI_MFMA_ASM(c2); GPMI_MFMA_ASM(c3);
        GPMI_MFMA_ASM(c4); GPMI_MFMA_ASM(c5); GPMI_MFMA_ASM(c6); GPMI_MFMA_ASM(c7);
    }
    asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");
#undef GPMI_MFMA_ASM
    d4 s = c0 + c1 + c2 + c3 + c4 + c5 + c6 + c7;
    const unsigned long long t1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
    if (s[0] + s[1] + s[2] + s[3] == 123.456) sink[0] = s[0];
    if (l == 0) {  // shader clock = d(s_memtime) / d(s_memrealtime) * 100 MHz
        sink[8 + 2 * blockIdx.x] = (double)(t1 - t0);
        sink[9 + 2 * blockIdx.x] = (double)(r1 - r0);
    }
}
#endif  // GPMI_PROBES

}  // namespace

// ---------------------------------------------------------------------------
// host-side drivers
// ---------------------------------------------------------------------------
void gpmi_tuning_defaults(gpmi_tuning *t)
{
    t->syrk_order = 2;
    t->stagger = (2 << 16) | 4;
    t->fuse_diag = 15;
    t->nb_adapt = 1;
    t->nb_thr[0] = 8192;
    t->nb_thr[1] = 4608;
    t->nb_thr[2] = 3584;
    t->ksplit = 1;
    t->ksplit_max = 100;
    t->block_recursive = 1;
    t->debug_ncu = 0;     // test hook: the trailing-update planner sees the device's own CU count
    t->se_nt = 1;
    t->small_n = 256;
    t->small_n1 = 128;
    t->small_m = 160;
    t->small_ng1 = 128;   // tools/grad_small_bench.py: one workgroup 57 / 82 / 109 / 207 / 303 / 337 us at n = 21 / 64 / 128 / 160 / 199 / 256,
                          // the launch chain 151 / 162 / 180 / ~225 / 274 / 272; four chains at once 93 .. 363 us against 377 .. 525
    t->small_ng = 256;
    t->grad_aug_n = 3072;
    t->grad_aug_ng = 2304;
    t->small_vjp = 256;
    t->small_cen = 192;   // tools/centered_gp_bench.py (k = 2, normal_logsd, m = 5): one workgroup 68 / 100 / 144 / 261 / 306 / 363 / 392 us at
                          // n = 10 / 64 / 128 / 160 / 192 / 224 / 256, the blocked chain 188 / 206 / 236 / 309 / 323 / 338 / 339
    t->small_gc = 180;    // gpmi_gp_condition by one workgroup up to n + m + 1 rows (tools/cond_bench.py)
    t->small_pr = 180;    // gpmi_gp_predict by one workgroup up to n + m + 1 rows (tools/predict_bench.py)
    t->small_pj = 300;    // gpmi_gp_predict_joint by one workgroup up to n + m + 1 rows: the crossover at B = 1 (tools/predict_joint_bench.py)
    t->small_jp = 220;    // gpmi_joint_predict by one workgroup up to 2n + p m + 1 rows: the crossover at B = 1, p = 3 (tools/joint_predict_bench.py
                          // --crossover: 165 / 187 us one workgroup / chain at 201 rows, 265 / 228 at 251)
    t->predict_mb = 0;   // rows of Xs per chunk of the blocked prediction chain (0: auto, about n / 4)
    t->small_sd = 640;
    t->small_sdb = 5;     // tools/sample_derivs_bench.py: one workgroup 0.21 / 0.56 / 0.73 ms at n = m = 79 / 199 / 256, the lanes 95 / 136 / 129 us per draw
    t->small_n2 = 1024;
    t->small_g2 = 40;
}

void launch_gemm_nt(const gpmi_ctx *c, hipStream_t s, const double *A, size_t lda, const double *B, size_t ldb,
                    double *C, size_t ldc, int M, int N, int K, int accumulate_minus)
{
    if (M <= 0 || N <= 0 || K <= 0) return;
    dim3 grid((M + GT - 1) / GT, (N + GT - 1) / GT);
    if (accumulate_minus)
        hipLaunchKernelGGL(k_gemm_nt<0>, grid, 256, 0, s, A, lda, B, ldb, C, ldc, M, N, K, 0, 0, FuseDiag{}, KSplit{});
    else
        hipLaunchKernelGGL(k_gemm_nt<2>, grid, 256, 0, s, A, lda, B, ldb, C, ldc, M, N, K, 0, 0, FuseDiag{}, KSplit{});
}

// C (n x n, lower tiles only; the caller zeroes the rest) = A B^T, A lower triangular, B the transpose of a lower
// triangular matrix: n^3 / 3 flops instead of 2 n^3
void launch_gemm_tri_lower(hipStream_t s, const double *A, size_t lda, const double *B, size_t ldb, double *C, size_t ldc, int n)
{
    if (n <= 0) return;
    const int T = (n + GT - 1) / GT;
    hipLaunchKernelGGL(k_gemm_nt<2>, dim3(syrk_grid(T, T)), 256, 0, s, A, lda, B, ldb, C, ldc, n, n, n, 0x400, 0, FuseDiag{},
                       KSplit{});
}

// the next panel's diagonal block is factored inside the update that completes it -- bit 0: in-block
// GEMMs, bit 1: the trailing SYRK (multi-round launches only).  Measured with 4 grid lanes (N = 16384 /
// 8192, ms per evaluation): off 25.0 / 4.12, GEMMs only 25.25 / 4.12, SYRK only 24.95 / 4.07, both
// 24.55 / 4.02 -- with both, no one-workgroup kernel is left that has to find a free CU next to the
// other lanes' updates.  One evaluation at a time: neutral (the block's tile sits on the critical
// path either way).
// (tune.fuse_diag, default 15; bit 2: sub-tiled diagonal tile in the fused in-block GEMMs; bit 3: the same in
// single-round trailing SYRK launches)

// C -= A B^T with the default kernel and the diagonal block at C's origin factored by the
// workgroup of tile (0, 0).  false: this configuration cannot fuse (caller launches the
// diagonal kernel itself and uses launch_gemm_nt).
static bool launch_gemm_nt_fused(const gpmi_ctx *c, hipStream_t s, const double *A, size_t lda, const double *B, size_t ldb, double *C,
                                 size_t ldc, int M, int N, int K, const FuseDiag &fd)
{
    if (!(c->tune.fuse_diag & 1) || M <= 0 || N <= 0 || K <= 0) return false;
    dim3 grid((M + GT - 1) / GT, (N + GT - 1) / GT);
    if ((c->tune.fuse_diag & 4) && fd.ctr && M >= GT && N >= GT && K % 64 == 0) {  // tile (0, 0) interior: sub-tiled
        hipLaunchKernelGGL(k_gemm_nt<0>, dim3(grid.x * grid.y + SUBWG - 1), 256, 0, s, A, lda, B, ldb, C, ldc, M, N, K, 0x200, 0, fd, KSplit{});
        return true;
    }
    hipLaunchKernelGGL(k_gemm_nt<0>, grid, 256, 0, s, A, lda, B, ldb, C, ldc, M, N, K, 0, 0, fd, KSplit{});
    return true;
}

// tune.nb_adapt    1 (default): the auto outer-block width is re-chosen per block from the order of the matrix still to
//                  update (tune.nb_thr: >= 8192 -> 1024 columns, >= 4608 -> 512, >= 3584 -> 256, below -> 128): the last
//                  blocks of a large matrix are a small matrix.  Pays since single-round trailing updates carry the next
//                  diagonal block (fuse_diag bit 3): N = 8192 5.63 -> 5.35 ms one at a time, 3.54 -> 3.38 on lanes;
//                  N = 4096 1.54 -> 1.47; N = 16384 28.0 -> 27.4 / 23.3 -> 23.1 (thresholds swept in steps of 1024)
// the CU count the trailing-update planner sees: the device's, or the "debug_ncu" test hook's
static int plan_ncu(const gpmi_ctx *c) { return c->tune.debug_ncu > 0 ? c->tune.debug_ncu : c->ncu; }

// C(lower) -= P P^T by the plan of syrk_plan (syrk_walk.h: tile walk, tail split, fused diagonal block); returns the plan --
// .fuse: fd was given and the launch factors the diagonal block at C's origin
static SyrkPlan launch_syrk_lower(const gpmi_ctx *c, hipStream_t s, const double *P, size_t ldp, double *C, size_t ldc, int M,
                                  int N, int K, int ncu, int tri = 0, const FuseDiag *fd = nullptr)
{
    // the sub-tiled single-round fusion (bit 3) needs the context's counter
    const SyrkTune tune{c->tune.syrk_order, c->tune.stagger, c->d_ctr ? c->tune.fuse_diag : (c->tune.fuse_diag & ~8), c->tune.ksplit,
                        c->tune.ksplit_max};
    const SyrkPlan p = syrk_plan(M, N, K, syrk_slots(ncu), tune, c->lanes_active, fd && fd->Fp, tri);
    if (!p.launch) return p;
    FuseDiag fdl = p.fuse ? *fd : FuseDiag{};
    if (p.order & 0x200) fdl.ctr = c->d_ctr + 8;
    hipLaunchKernelGGL(k_gemm_nt<1>, dim3(p.grid), 256, 0, s, P, ldp, P, ldp, C, ldc, M, N, K, p.order, p.stagger, fdl, p.ks);
    return p;
}

#ifdef GPMI_PROBES
void launch_syrk_probe(const gpmi_ctx *c, hipStream_t s, const double *P, size_t ldp, double *C, size_t ldc, int m, int k)
{
    launch_syrk_lower(c, s, P, ldp, C, ldc, m, m, k, plan_ncu(c));
}
#endif

// C(lower) -= U U^T for an upper-triangular n x n U
void launch_syrk_uut(const gpmi_ctx *c, hipStream_t s, const double *U, size_t ldu, double *C, size_t ldc, int n)
{
    launch_syrk_lower(c, s, U, ldu, C, ldc, n, n, n, 0, 1);
}

// C(lower) -= P P^T for a full n x n P: the trailing update's launch (tile walk, tail split) with nothing fused
void launch_syrk_ppt(const gpmi_ctx *c, hipStream_t s, const double *P, size_t ldp, double *C, size_t ldc, int n)
{
    launch_syrk_lower(c, s, P, ldp, C, ldc, n, n, n, plan_ncu(c));
}

// tune.block_recursive  1: in-block updates by recursive halving; 0: 128 / 256 / rest-of-block levels

// One 128-column panel [k, k + kb): diagonal block, then the rows [max(k + kb, row_lo), row_hi) below it.
static double *fpack_slot(gpmi_ctx *c, double *Fpack_all, int ko, int k)
{
    return Fpack_all ? Fpack_all + (size_t)(k / GPMI_NB) * GPMI_FPACK
                     : c->Fpack + (size_t)(((k - ko) / GPMI_NB) % GPMI_FPACK_SLOTS) * GPMI_FPACK;
}

static void panel_one(gpmi_ctx *c, double *W, size_t ld, int *d_info, double *Fpack_all, int ko, int k, int kb,
                      int row_lo, int row_hi, bool with_diag, hipStream_t s)
{
    double *Fp = fpack_slot(c, Fpack_all, ko, k);
    if (with_diag)
        hipLaunchKernelGGL(k_potrf_diag4, dim3(1), 256, 0, s, W + (size_t)k + (size_t)k * ld, ld, kb, Fp, d_info, k);
    const int r0 = k + kb;
    const int rlo = r0 > row_lo ? r0 : row_lo;
    if (rlo >= row_hi) return;
    hipLaunchKernelGGL(k_trsm_panel, dim3((row_hi - rlo + 63) / 64), 256, 0, s, W + (size_t)k * ld, ld, rlo, row_hi, kb, Fp);
}

// Columns [k0, k1) by recursive halving at panel boundaries: factor the left half, update the
// right half with it in ONE product (K = width of the left half: 128, 256, 512 for a 1024-column
// block), factor the right half.  Compared with fixed 128 / 256 levels the same flops move from
// K = 256 products to a K = 512 one, whose per-tile prologue and C round trip weigh half as much.
static void panel_rec(gpmi_ctx *c, double *W, size_t ld, int *d_info, double *Fpack_all, int ko, int k0, int k1,
                      int row_lo, int row_hi, bool with_diag, bool first_diag_done, hipStream_t s)
{
    const int NB = GPMI_NB;
    if (k1 - k0 <= NB) {
        panel_one(c, W, ld, d_info, Fpack_all, ko, k0, k1 - k0, row_lo, row_hi, with_diag && !first_diag_done, s);
        return;
    }
    const int npan = (k1 - k0 + NB - 1) / NB;
    const int km = k0 + ((npan + 1) / 2) * NB;
    panel_rec(c, W, ld, d_info, Fpack_all, ko, k0, km, row_lo, row_hi, with_diag, first_diag_done, s);
    const int rlo = km > row_lo ? km : row_lo;
    bool fused = false;
    if (rlo < row_hi) {  // rows [rlo, row_hi) x cols [km, k1) -= A[rows, k0:km] A[km:k1, k0:km]^T
        const double *A = W + (size_t)rlo + (size_t)k0 * ld, *B = W + (size_t)km + (size_t)k0 * ld;
        double *C = W + (size_t)rlo + (size_t)km * ld;
        if (with_diag && rlo == km) {  // C starts at the next panel's diagonal block: factor it in this launch
            const int kb = (k1 - km < NB) ? k1 - km : NB;
            fused = launch_gemm_nt_fused(c, s, A, ld, B, ld, C, ld, row_hi - rlo, k1 - km, km - k0,
                                         FuseDiag{fpack_slot(c, Fpack_all, ko, km), d_info, km, kb, c->d_ctr + 8});
        }
        if (!fused) launch_gemm_nt(c, s, A, ld, B, ld, C, ld, row_hi - rlo, k1 - km, km - k0, 1);
    }
    panel_rec(c, W, ld, d_info, Fpack_all, ko, km, k1, row_lo, row_hi, with_diag, fused, s);
}

// Panel work of one outer block [ko, ke) restricted to the rows [row_lo, row_hi) below each
// panel.  with_diag: also factor the 128 x 128 diagonal blocks (their factors go to the block's
// Fpack slots); without it the slots written by an earlier call are used.
//   (0, M, true)   : the whole panel phase, full height
//   (0, ke, true)  : only the NBO x NBO diagonal block -- the latency chain
//   (ke, M, false) : the rows below it -- wide, throughput-bound kernels
// tune.block_recursive == 0 keeps the earlier three fixed levels: 128-column panels grouped into
// middle blocks of NBM columns; a panel's K = 128 update reaches only to the end of its middle
// block, the rest of the outer block is updated once per middle block with K = NBM.
static void panel_rows(gpmi_ctx *c, double *W, size_t ld, int *d_info, double *Fpack_all, int ko, int ke, int NBO,
                       int row_lo, int row_hi, bool with_diag, hipStream_t s, bool first_diag_done = false)
{
    if (c->tune.block_recursive) {
        panel_rec(c, W, ld, d_info, Fpack_all, ko, ko, ke, row_lo, row_hi, with_diag, first_diag_done, s);
        return;
    }
    const int NB = GPMI_NB;
    const int NBM = (NBO >= 512) ? 256 : NBO;
    for (int km = ko; km < ke; km += NBM) {
        const int kme = (km + NBM < ke) ? km + NBM : ke;
        for (int k = km; k < kme; k += NB) {
            const int kb = (kme - k < NB) ? kme - k : NB;
            panel_one(c, W, ld, d_info, Fpack_all, ko, k, kb, row_lo, row_hi, with_diag && !(first_diag_done && k == ko), s);
            const int r0 = k + kb;
            const int rlo = r0 > row_lo ? r0 : row_lo;
            if (rlo >= row_hi) continue;
            if (r0 < kme)  // rest of this middle block: rows [rlo, row_hi) x cols [r0, kme), K = kb
                launch_gemm_nt(c, s, W + (size_t)rlo + (size_t)k * ld, ld, W + (size_t)r0 + (size_t)k * ld, ld,
                               W + (size_t)rlo + (size_t)r0 * ld, ld, row_hi - rlo, kme - r0, kb, 1);
        }
        const int rlo = kme > row_lo ? kme : row_lo;
        if (kme < ke && rlo < row_hi)  // rest of the outer block: cols [kme, ke), K = kme - km
            launch_gemm_nt(c, s, W + (size_t)rlo + (size_t)km * ld, ld, W + (size_t)kme + (size_t)km * ld, ld,
                           W + (size_t)rlo + (size_t)kme * ld, ld, row_hi - rlo, ke - kme, kme - km, 1);
    }
}

int launch_potrf_partial(gpmi_ctx *c, double *W, size_t ld, int M, int ncol, int nfac, int *d_info,
                         double *Fpack_all)
{
    // Blocked right-looking factorisation of the leading nfac columns of the M x ncol lower
    // trapezoid in W; the trailing [nfac, ncol) part receives the Schur complement.
    // outer block width: K of the trailing update.  Wider blocks cut the C traffic and the
    // number of epilogues once the trailing matrix is large; 256 keeps the panel phase short.
    // small matrices: the whole partial factorisation in ONE workgroup of one launch (k_potrf_small) instead of a
    // chain of latency-bound launches (tune.small_m; callers that keep the packed factors take the blocked path)
    if (!Fpack_all && M <= c->tune.small_m && M > 0 && nfac > 0) {
        launch_potrf_small(c->stream, W, ld, M, ncol, nfac, d_info);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return gpmi_fail(GPMI_EHIP, "potrf launch failed: %s", hipGetErrorString(e));
        return 0;
    }
    auto nbo_for = [c](int cols) {
        return cols >= c->tune.nb_thr[0] ? 1024 : (cols >= c->tune.nb_thr[1] ? 512 : (cols >= c->tune.nb_thr[2] ? 256 : 128));
    };
    const int NBO = c->nb_outer > 0 ? c->nb_outer : nbo_for(ncol);
    hipStream_t s = c->stream;
    // auto width follows the order of the matrix still to update (tune.nb_adapt): the last blocks of a
    // large matrix are a small matrix, whose few trailing tiles do not fill the chip at K = 1024
    bool diag_done = false;
    for (int ko = 0, nbo = NBO; ko < nfac; ko += nbo) {
        nbo = (c->nb_outer > 0 || !c->tune.nb_adapt) ? NBO : nbo_for(ncol - ko);
        const int ke = (ko + nbo < nfac) ? ko + nbo : nfac;
        kt_begin(c, 2, s);
        panel_rows(c, W, ld, d_info, Fpack_all, ko, ke, nbo, 0, M, true, s, diag_done);
        {   // algorithmic flops of the panel phase: diagonal block w^3/3 + rows below (m - w) w^2
            const double w = (double)(ke - ko), m = (double)(M - ko);
            kt_end(c, 2, w * w * (m - w) + w * w * w / 3.0, s);
        }
        diag_done = false;
        if (ke >= M || ke >= ncol) continue;
        const double mt = (double)(ncol - ke), extra = (double)(M - ncol);
        // the first diagonal block of the next outer block rides in this trailing update
        FuseDiag fd{};
        if (ke < nfac)
            fd = FuseDiag{fpack_slot(c, Fpack_all, ke, ke), d_info, ke, (nfac - ke < GPMI_NB) ? nfac - ke : GPMI_NB, nullptr};
        kt_begin(c, 1, s);
        const SyrkPlan plan = launch_syrk_lower(c, s, W + (size_t)ke + (size_t)ko * ld, ld, W + (size_t)ke + (size_t)ke * ld, ld, M - ke,
                                                ncol - ke, ke - ko, plan_ncu(c), 0, &fd);
        diag_done = plan.fuse;
        // algorithmic flops: lower triangle (incl. diagonal) of the square part + extra rows; flag: more than one round of
        // tiles (throughput-bound launch)
        kt_end(c, 1, (mt * (mt + 1.0) + 2.0 * extra * mt) * (double)(ke - ko), s, plan.multi_round);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return gpmi_fail(GPMI_EHIP, "potrf launch failed: %s", hipGetErrorString(e));
    return 0;
}

// Columns [c0, c1) of X <- X L^-T by recursive halving at panel boundaries: solve the left half, take
// it out of the right half in ONE product (K = width of the left half: the bulk of the N^3 flops runs
// at K in the thousands instead of K = 128), solve the right half.  upper_tri: X[i][j] = 0 for i > j --
// column block [c0, c1) has rows [0, c1) only, and the product skips the zero columns of its
// trapezoidal A operand per row-tile.
static void trsm_right_rec(const gpmi_ctx *c, hipStream_t s, const double *L, size_t ldl, double *X, size_t ldx, int mrows,
                           const double *Fpack_all, int upper_tri, int c0, int c1)
{
    const int NB = GPMI_NB;
    const bool lower_out = upper_tri == 2;  // only the rows >= a column block's first column are wanted (and kept valid)
    if (c1 - c0 <= NB) {
        const int mr = (upper_tri == 1 && c1 < mrows) ? c1 : mrows;
        const int r0 = lower_out ? c0 : 0;
        if (r0 < mr)
            hipLaunchKernelGGL(k_trsm_panel, dim3((mr - r0 + 63) / 64), 256, 0, s, X + (size_t)c0 * ldx, ldx, r0, mr, c1 - c0,
                               Fpack_all + (size_t)(c0 / NB) * GPMI_FPACK);
        return;
    }
    const int npan = (c1 - c0 + NB - 1) / NB;
    const int cm = c0 + ((npan + 1) / 2) * NB;
    trsm_right_rec(c, s, L, ldl, X, ldx, mrows, Fpack_all, upper_tri, c0, cm);
    const int mr = (upper_tri == 1 && cm < mrows) ? cm : mrows;  // rows where X[:, c0:cm] is non-zero
    const int r0 = lower_out ? cm : 0;                           // rows of the right half that are wanted
    const double *A = X + (size_t)r0 + (size_t)c0 * ldx, *B = L + (size_t)cm + (size_t)c0 * ldl;
    double *C = X + (size_t)r0 + (size_t)cm * ldx;
    if (upper_tri == 1) {
        dim3 grid((c1 - cm + GT - 1) / GT, (mr + GT - 1) / GT);  // x: column tiles, y: row tiles (long K first)
        hipLaunchKernelGGL(k_gemm_nt<0>, grid, 256, 0, s, A, ldx, B, ldl, C, ldx, mr, c1 - cm, cm - c0, 0x100, 0,
                           FuseDiag{nullptr, nullptr, c0, 0, nullptr}, KSplit{});
    } else if (mr > r0) {
        launch_gemm_nt(c, s, A, ldx, B, ldl, C, ldx, mr - r0, c1 - cm, cm - c0, 1);
    }
    trsm_right_rec(c, s, L, ldl, X, ldx, mrows, Fpack_all, upper_tri, cm, c1);
}

int launch_trsm_right(gpmi_ctx *c, const double *L, size_t ldl, int n, double *X, size_t ldx,
                      int mrows, const double *Fpack_all, int upper_tri)
{
    // X <- X L^-T by block forward substitution over the 128-column panels.  upper_tri = 1: X is
    // upper triangular on entry (e.g. the identity) and stays so -- panel k then only has rows
    // [0, k + kb), which cuts the work to a third.  upper_tri = 2: only the LOWER triangle of the result is
    // wanted (rows >= the column's block start; the rest of X is left half-updated): the rows of a column block
    // need, from the blocks to their left, those same rows only -- also a third of the work.
    hipStream_t s = c->stream;
    const int NB = GPMI_NB;
    // many right-hand rows: products with large K.  For a triangular X the recursion pays from
    // N ~ 12k on (value + gradient at N = 16384: 88.9 -> 83.2 ms; N = 8192: 16.0 vs 16.5 ms, N = 4096:
    // 4.5 vs 5.2 ms -- unequal tile lengths and more launches)
    if (mrows >= 2 * GT && n > NB && (upper_tri != 1 || n >= 12288)) {
        trsm_right_rec(c, s, L, ldl, X, ldx, mrows, Fpack_all, upper_tri, 0, n);
    } else {  // a few rows (triangular solve of vectors): one pass over L, panel by panel
        for (int k = 0; k < n; k += NB) {
            const int kb = (n - k < NB) ? n - k : NB;
            const double *Fp = Fpack_all + (size_t)(k / NB) * GPMI_FPACK;
            const int mr = (upper_tri == 1 && k + kb < mrows) ? k + kb : mrows;  // (lower-only output: everything, it is small)
            hipLaunchKernelGGL(k_trsm_panel, dim3((mr + 63) / 64), 256, 0, s, X + (size_t)k * ldx, ldx, 0, mr, kb, Fp);
            const int r0 = k + kb;
            if (r0 < n)
                launch_gemm_nt(c, s, X + (size_t)k * ldx, ldx, L + (size_t)r0 + (size_t)k * ldl, ldl,
                               X + (size_t)r0 * ldx, ldx, mr, n - r0, kb, 1);
        }
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return gpmi_fail(GPMI_EHIP, "trsm launch failed: %s", hipGetErrorString(e));
    return 0;
}

// Dinv (ceil(n / 128) blocks of 128 x 128 doubles): inverses of L's diagonal blocks from its packed factors;
// tmp: the same size of scratch
void launch_diag_inverses(hipStream_t s, const double *Fpack_all, int n, double *Dinv, double *tmp)
{
    if (n <= 0) return;
    const int nblk = (n + TSV - 1) / TSV;
    hipLaunchKernelGGL(k_eye_blocks, dim3(nblk), 256, 0, s, tmp, nblk);
    for (int w = 0; w < nblk; ++w) {
        const int kb = (n - w * TSV < TSV) ? n - w * TSV : TSV;
        hipLaunchKernelGGL(k_trsm_panel, dim3(2), 256, 0, s, tmp + (size_t)w * TSV * TSV, (size_t)TSV, 0, TSV, kb,
                           Fpack_all + (size_t)w * GPMI_FPACK);
    }
    hipLaunchKernelGGL(k_transpose_blocks, dim3(nblk, 64), 256, 0, s, tmp, Dinv);
}

// t = L^-1 k (k, t: n contiguous doubles, different buffers) in one launch; Dinv from launch_diag_inverses
int launch_trsv_lower(hipStream_t s, const double *L, size_t ldl, int n, const double *k, double *t, const double *Dinv,
                      int *ticket /* zeroed device int owned by the calling context; left zero */)
{
    if (n <= 0) return 0;
    hipError_t e = hipMemsetAsync(t, 0xff, (size_t)n * sizeof(double), s);  // "not yet" in every element
    if (e != hipSuccess) return gpmi_fail(GPMI_EHIP, "memset failed: %s", hipGetErrorString(e));
    hipLaunchKernelGGL(k_trsv_wave, dim3((n + TSV - 1) / TSV), 256, 0, s, L, ldl, n, k, t, Dinv, ticket);
    e = hipGetLastError();
    if (e != hipSuccess) return gpmi_fail(GPMI_EHIP, "trsv launch failed: %s", hipGetErrorString(e));
    return 0;
}

void launch_pack_factors(hipStream_t s, const double *L, size_t ldl, int n, double *Fpack_all)
{
    for (int k = 0; k < n; k += GPMI_NB) {
        const int kb = (n - k < GPMI_NB) ? n - k : GPMI_NB;
        hipLaunchKernelGGL(k_pack_factors, dim3(1), 512, 0, s, L + (size_t)k + (size_t)k * ldl, ldl, kb,
                           Fpack_all + (size_t)(k / GPMI_NB) * GPMI_FPACK);
    }
}

void launch_get_row(hipStream_t s, const double *W, size_t ld, int row, int col0, int m, double scale, double *out)
{
    if (m <= 0) return;
    hipLaunchKernelGGL(k_get_row, dim3((m + 255) / 256), 256, 0, s, W, ld, row, col0, m, scale, out);
}

// part: 2 * ceil(n / 256) doubles of scratch
void launch_logml_finalize(hipStream_t s, const double *W, size_t ld, int n, int zrow,
                           const int *d_info, double *d_out3, int *d_info_out, double *part)
{
    const int nslice = (n + FIN_SLICE - 1) / FIN_SLICE;
    hipLaunchKernelGGL(k_logml_partial, dim3(nslice), FIN_SLICE, 0, s, W, ld, n, zrow, part);
    hipLaunchKernelGGL(k_logml_finalize, dim3(1), 256, 0, s, part, nslice, n, d_info, d_out3, d_info_out);
}

int trmv_lower_chunks(int n) { return (n + TMV_COLS - 1) / TMV_COLS; }

// part: trmv_lower_chunks(n) * n doubles of scratch
void launch_trmv_lower(hipStream_t s, const double *L, size_t ldl, int n, const double *z, double *f, double *part)
{
    if (n <= 0) return;
    const int nchunk = trmv_lower_chunks(n);
    hipLaunchKernelGGL(k_trmv_lower_part, dim3((n + 255) / 256, nchunk), 256, 0, s, L, ldl, n, z, part);
    hipLaunchKernelGGL(k_trmv_lower_sum, dim3((n + 255) / 256), 256, 0, s, part, n, nchunk, f);
}

void launch_trmv_lower_t(hipStream_t s, const double *L, size_t ldl, int n, const double *u, size_t ldu, double *w, size_t ldw, int k)
{
    if (n <= 0 || k <= 0) return;
    hipLaunchKernelGGL(k_trmv_lower_t, dim3((n + 3) / 4, k), 256, 0, s, L, ldl, n, u, ldu, w, ldw);
}

#ifdef GPMI_PROBES
int probe_fused_read(hipStream_t s, unsigned long long *out5)
{
    unsigned long long z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (hipStreamSynchronize(s) != hipSuccess) return 1;
    if (hipMemcpyFromSymbol(out5, HIP_SYMBOL(g_fz), 8 * sizeof(unsigned long long)) != hipSuccess) return 1;
    return hipMemcpyToSymbol(HIP_SYMBOL(g_fz), z, sizeof z) != hipSuccess;
}

int probe_small_body_read(hipStream_t s, unsigned long long *out8);
// the bodies of both translation units: the blocked launches' (this file's g_body) and the one-workgroup kernels'
int probe_body_read(hipStream_t s, unsigned long long *out8)
{
    unsigned long long z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (hipStreamSynchronize(s) != hipSuccess) return 1;
    if (hipMemcpyFromSymbol(out8, HIP_SYMBOL(g_body), 8 * sizeof(unsigned long long)) != hipSuccess) return 1;
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_body), z, sizeof z) != hipSuccess) return 1;
    unsigned long long sm[8];
    if (probe_small_body_read(s, sm)) return 1;
    for (int i = 0; i < 8; ++i) out8[i] += sm[i];
    return 0;
}

int probe_clock_read(hipStream_t s, int reset, unsigned long long *out3)
{
    unsigned long long h[4] = {0, 0, 0, 0};
    if (hipStreamSynchronize(s) != hipSuccess) return 1;
    if (hipMemcpyFromSymbol(h, HIP_SYMBOL(g_clk), sizeof h) != hipSuccess) return 1;
    for (int i = 0; i < 3; ++i) out3[i] = h[i];
    if (reset) {
        unsigned long long z[4] = {0, 0, 0, 0};
        if (hipMemcpyToSymbol(HIP_SYMBOL(g_clk), z, sizeof z) != hipSuccess) return 1;
    }
    return 0;
}

void launch_probe_mfma(hipStream_t s, const double *A, const double *B, double *D)
{
    hipLaunchKernelGGL(k_probe_mfma, dim3(1), 64, 0, s, A, B, D);
}

void launch_probe_peak(hipStream_t s, double *sink, int iters, int *blocks, int *threads)
{
    *blocks = 256 * 4;
    *threads = 256;
    hipLaunchKernelGGL(k_probe_peak, dim3(*blocks), 256, 0, s, sink, iters);
}
#endif  // GPMI_PROBES
