// Device functions of the blocked fp64 Cholesky that more than one translation unit inlines: the blocked kernels of
// chol_kernels.hip and the one-workgroup kernels of small_kernels.hip run the SAME diagonal-block body, panel-solve body
// and tile products (chol_kernels.hip's header comment states the tile layout they share).  Everything here is
// __forceinline__ device code in an anonymous namespace: each translation unit compiles its own copy (the build has no
// relocatable device code), and in the probe build each has its own g_body stamp array.
#pragma once
#include "gpmi_internal.h"
#include "syrk_walk.h"
#include <math.h>
#include <type_traits>

namespace {

__device__ __forceinline__ d4 mfma(double a, double b, d4 c)
{
    return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
}

// C-tile accesses of the update kernels: dbg bit 3 (probe) makes them non-temporal so that the
// streamed C tiles do not displace the panel operands, which every tile re-reads, from L2
__device__ __forceinline__ double ld_c(const double *p, bool nt) { return nt ? __builtin_nontemporal_load(p) : *p; }
__device__ __forceinline__ void st_c(double *p, double v, bool nt)
{
    if (nt) __builtin_nontemporal_store(v, p);
    else *p = v;
}

__device__ __forceinline__ double readlane64(double v, int l)
{
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __builtin_amdgcn_readlane(lo, l);
    hi = __builtin_amdgcn_readlane(hi, l);
    return __hiloint2double(hi, lo);
}

// Fpack tile slots (256 doubles each): negated L block (jb,kb), kb<jb, then Linv16 of block jb
__device__ __host__ constexpr int fp_l(int jb, int kb) { return jb * (jb - 1) / 2 + kb; }
__device__ __host__ constexpr int fp_inv(int jb) { return 28 + jb; }


#include "factor16.h"

// ---------------------------------------------------------------------------
// Diagonal block, 4-wave variant: the same algorithm with THREE tile waves (block-rows
// {7,2,0}, {6,3,1}, {5,4}: 12 / 13 / 11 register tiles) and the factor wave.  One wave per
// SIMD and ~50 KB of LDS: the workgroup fits into the half of a CU that a retiring
// trailing-update workgroup leaves behind, so next to a running SYRK it starts within
// microseconds instead of waiting for a whole CU to drain by chance (5 waves need two wave
// slots with ~200 registers each on one SIMD, which a resident SYRK wave rules out).
// ---------------------------------------------------------------------------
#ifdef GPMI_PROBES
// where a diagonal-block body spends its cycles (accumulated over all bodies since the last read): [0] block loads
// (drained), [1] the 8-step loop, [2] stores, [3] factor wave inside factor16, [4] factor wave waiting at B1 for the
// next diagonal tile, [5] bodies
__device__ unsigned long long g_body[8];
#define GPMI_BSTAMP(v) const unsigned long long v = __builtin_amdgcn_s_memtime();
#define GPMI_BADD(i, d) atomicAdd(&g_body[i], (unsigned long long)(d));
#else
#define GPMI_BSTAMP(v)
#define GPMI_BADD(i, d)
#endif
template <bool COH>
__device__ __forceinline__ double ld_blk(const double *p)
{
    if constexpr (COH) return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else return *p;
}
constexpr int DIAG4_LDS = 2 * 8 * 256 + 8 * 256 + 2 * 16 * 17 + 2;  // doubles of workgroup memory the body needs (52 KB; the last two: the tile waves' arrival counter)
// COH: the block was written by other workgroups of the same launch with agent-scope stores; read it
// with agent-scope loads (they do not trust this XCD's L2) instead of invalidating caches with a fence
// FULL: the block has all 128 rows and columns (every panel but a ragged last one): the tiles below the
// diagonal are loaded and stored unconditionally -- the guarded form costs a compare, an exec-mask
// save / restore and a branch per ELEMENT (60 per lane), ~3 us per block
// nblk (ragged blocks only): number of 16-column pivot blocks to run, ceil(nb_act / 16) -- a small matrix does not
// pay for the identity padding's pivots (n = 21: 2 of 8 block columns); Fpack slots of the skipped blocks are then
// never read by the consumers, which loop over the same count
template <bool COH = false, bool FULL = false>
__device__ __forceinline__ void potrf_diag4_body(double *__restrict__ sm, double *__restrict__ A, size_t lda, int nb_act,
                                                 double *__restrict__ Fpack, int *info, int col0, int nblk = 8,
                                                 int tid = (int)threadIdx.x)
{
    if (FULL) nblk = 8;
    // ragged blocks: block-rows >= nblk are identity padding -- not loaded, solved, updated or stored (at n = 21 two of
    // eight block-rows exist; carrying the padding through every step was half of the body's time there)
#define GPMI_ACT(br) (FULL || (br) < nblk)
    double (*s_pub)[8][256] = reinterpret_cast<double (*)[8][256]>(sm);
    double (*s_inv)[256] = reinterpret_cast<double (*)[256]>(sm + 2 * 8 * 256);
    // the diagonal tile travels to the factor wave and comes back as L16 through s_d16[kb & 1]: two
    // buffers, so that the owner of block-row kb + 1 can hand over the NEXT diagonal tile while the
    // owner of block-row kb still reads L16 of this step
    double (*s_d16)[16][17] = reinterpret_cast<double (*)[16][17]>(sm + 2 * 8 * 256 + 8 * 256);
    const int lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lr = lane & 15, lq = lane >> 4;

    // TWO workgroup barriers per block column.  The chain factor16(kb) -> solve of block-row kb + 1 ->
    // update of its diagonal tile -> factor16(kb + 1) crosses B2 and B1 only: the update of the next
    // diagonal tile needs nothing but its owner's own solve result (register r of X is, lane for lane,
    // the A and the B operand of X X^T), so no barrier stands between the solve and that update (the
    // third barrier of the earlier form cost ~2 k of the ~7.7 k cycles per step).
    // The barriers order LDS traffic only (the waves talk through s_d16 / s_inv / s_pub): they are raw
    // s_waitcnt lgkmcnt(0) + s_barrier, NOT __syncthreads(), whose release fence also drains vmcnt -- so the block's
    // global loads may still be in flight at the first barriers (they are issued in the order they are needed: block
    // column 0 of every row first) and the finished tiles are stored from inside the loop, under the factor wave's
    // time, instead of in a ~6 k-cycle tail behind it.  Nothing in the body reads global memory another wave of the
    // workgroup has written.
#define GPMI_LDS_BARRIER() asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory")
    if (w == 3) {
#pragma unroll 1
        for (int kb = 0; kb < nblk; ++kb) {
            GPMI_BSTAMP(f0)
            GPMI_LDS_BARRIER();  // B1: the owner's diagonal tile is in s_d16[kb & 1]; -X tiles of step kb - 1 published
            GPMI_BSTAMP(f1)
            const int bad = factor16(s_d16[kb & 1], s_inv[kb], lane);
            if (bad && lane == 0) atomicCAS(info, 0, col0 + kb * 16 + bad);
            GPMI_BSTAMP(f2)
#ifdef GPMI_PROBES
            if (lane == 0) {
                GPMI_BADD(3, f2 - f1)
                GPMI_BADD(4, f1 - f0)
            }
#endif
            GPMI_LDS_BARRIER();  // B2: L16 in s_d16[kb & 1], L16^-1 in s_inv[kb]
        }
        return;
    }
    GPMI_BSTAMP(b0)

    // block-rows of this wave, ra > rb > rc (rc = -1: none); array sizes cover the largest row of each class
    const int ra = 7 - w, rb = 2 + w, rc = w < 2 ? w : -1;
    d4 TA[8], TB[5], TC[2];
#define GPMI_CL(jb, NJ) ((jb) < (NJ) ? (jb) : 0)  // keeps compile-time indices of never-taken branches in range
    // per block-row: A + (16 br + lr) + lq lda -- element (i) of tile jb is then a wave-uniform multiple of lda away
    // (the general form costs a max / min / 64-bit multiply-add per element: 4.5 k cycles of pure address arithmetic
    // for the 60 loads of a lane)
    const double *const pra = A + (size_t)(ra * 16 + lr) + (size_t)lq * lda;
    const double *const prb = A + (size_t)(rb * 16 + lr) + (size_t)lq * lda;
    const double *const prc = A + (size_t)((rc < 0 ? 0 : rc) * 16 + lr) + (size_t)lq * lda;
#define GPMI_LOAD_TILE(T, br, jb, PR)                                                                  \
    {                                                                                                  \
        T[jb] = d4{0.0, 0.0, 0.0, 0.0};                                                                \
        if (!GPMI_ACT(br)) {                                                                           \
        } else if (FULL && (jb) < (br)) {                                                              \
            _Pragma("unroll") for (int i = 0; i < 4; ++i) T[jb][i] = ld_blk<COH>(PR + (size_t)((jb) * 16 + 4 * i) * lda); \
        } else if ((jb) <= (br)) {                                                                     \
            _Pragma("unroll") for (int i = 0; i < 4; ++i) {                                            \
                const int col = (jb) * 16 + lq + 4 * i, row = (br) * 16 + lr;                          \
                const int rr = row > col ? row : col, cc = row > col ? col : row;                      \
                if (FULL) T[jb][i] = ld_blk<COH>(A + (size_t)rr + (size_t)cc * lda);                   \
                else T[jb][i] = (rr < nb_act) ? ld_blk<COH>(A + (size_t)rr + (size_t)cc * lda) : (row == col ? 1.0 : 0.0); \
            }                                                                                          \
        }                                                                                              \
    }
    // block column by block column, lowest rows first: tile (0, 0) and then the tiles of block column 0 are what the
    // first steps wait for
#pragma unroll
    for (int jb = 0; jb < 8; ++jb) {
        if (jb < 2) GPMI_LOAD_TILE(TC, rc, jb, prc)
        if (jb < 5) GPMI_LOAD_TILE(TB, rb, jb, prb)
        GPMI_LOAD_TILE(TA, ra, jb, pra)
    }

    // step k of block-row br: the diagonal tile comes back from the factor wave as L16; a row below is solved against
    // L16^-1 (4 chained MFMAs), keeps X as its final tile and publishes -X for the other rows' updates
#define GPMI_SOLVE_ROW(T, NJ, br, X, k)                                                                \
    if ((br) == (k)) {                                                                                 \
        _Pragma("unroll") for (int i = 0; i < 4; ++i) T[GPMI_CL(k, NJ)][i] = s_d16[(k) & 1][lr][lq + 4 * i]; \
    } else if ((br) > (k) && GPMI_ACT(br)) {                                                           \
        X = d4{0.0, 0.0, 0.0, 0.0};                                                                    \
        _Pragma("unroll") for (int kg = 0; kg < 4; ++kg)                                               \
            X = mfma(s_inv[k][kg * 64 + lane], T[GPMI_CL(k, NJ)][kg], X);                              \
        T[GPMI_CL(k, NJ)] = X;                                                                         \
        _Pragma("unroll") for (int kg = 0; kg < 4; ++kg) s_pub[(k) & 1][br][kg * 64 + lane] = -X[kg];  \
    }

    // The only tile the next pivot block waits for is the diagonal tile of block-row kb + 1: its
    // owner updates it first (EARLY), straight from the registers of its own solve, and hands it to
    // the factor wave; every other update of step kb (REST) runs in the next iteration between B1
    // and B2, i.e. under the factor wave's 4.4 k cycles.
#define GPMI_UPDATE_EARLY(T, NJ, br, X)                                                                \
    {                                                                                                  \
        _Pragma("unroll") for (int kg = 0; kg < 4; ++kg)                                               \
            T[GPMI_CL(kb + 1, NJ)] = mfma(-X[kg], X[kg], T[GPMI_CL(kb + 1, NJ)]);                      \
        _Pragma("unroll") for (int i = 0; i < 4; ++i) s_d16[(kb + 1) & 1][lr][lq + 4 * i] = T[GPMI_CL(kb + 1, NJ)][i]; \
    }
#define GPMI_UPDATE_REST(T, NJ, br, X)                                                                 \
    _Pragma("unroll") for (int jb = kb; jb < (NJ); ++jb) {                                             \
        if (jb <= (br) && !(jb == kb && (br) == kb)) {                                                 \
            _Pragma("unroll") for (int kg = 0; kg < 4; ++kg)                                           \
                T[jb] = mfma(s_pub[(kb - 1) & 1][jb][kg * 64 + lane], X[kg], T[jb]);                   \
        }                                                                                              \
    }
    // Block column k of block-row br is final once step k has solved it: L tile (from the solve's registers) and its
    // packed negative below the diagonal; on the diagonal the factor's tile and the inverse the factor wave left in
    // s_inv[k].  Issued one step later, behind B1, so that the stores do not sit between B2 and B1 (the critical path).
#define GPMI_STORE_STEP(T, NJ, br, k, PR)                                                              \
    if ((br) > (k) && !GPMI_ACT(br)) {                                                                 \
    } else if ((br) > (k)) {                                                                           \
        _Pragma("unroll") for (int i = 0; i < 4; ++i) {                                                \
            if (FULL || (br) * 16 + lr < nb_act)                                                       \
                const_cast<double *>(PR)[(size_t)((k) * 16 + 4 * i) * lda] = T[GPMI_CL(k, NJ)][i];     \
        }                                                                                              \
        _Pragma("unroll") for (int kg = 0; kg < 4; ++kg)                                               \
            Fpack[(size_t)fp_l(br, k) * 256 + kg * 64 + lane] = -T[GPMI_CL(k, NJ)][kg];                \
    } else if ((br) == (k)) {                                                                          \
        _Pragma("unroll") for (int i = 0; i < 4; ++i) {                                                \
            const int col = (k) * 16 + lq + 4 * i, row = (br) * 16 + lr;                               \
            if (col <= row && (FULL || row < nb_act)) A[(size_t)row + (size_t)col * lda] = T[GPMI_CL(k, NJ)][i]; \
        }                                                                                              \
        _Pragma("unroll") for (int kg = 0; kg < 4; ++kg)                                               \
            Fpack[(size_t)fp_inv(k) * 256 + kg * 64 + lane] = s_inv[k][kg * 64 + lane];                \
    }

    GPMI_BSTAMP(b1)
    // Between B2 (factor16 of step kb done) and B1 (the next diagonal tile handed over) -- the critical path -- ONLY the
    // owner of block-row kb + 1 works: it solves that row (4 MFMAs), updates the next diagonal tile from its own
    // registers (4 MFMAs) and hands it to the factor wave.  Every other solve of step kb, the publication of the -X
    // tiles, the stores and the REST updates run behind B1, under factor16(kb + 1); the REST updates read the other
    // rows' -X tiles, so the three tile waves meet once more in between, on an arrival counter in LDS (the factor
    // wave, busy on the chain, takes no part).  Before: all solves of a step stood between B2 and B1 (~2.0 k cycles
    // per step against ~0.9 k now).
    // (explicitly an LDS pointer: through a generic one the accesses become FLAT operations, whose completion the
    // compiler can only await with vmcnt(0) -- which would drain the block loads still in flight)
    typedef __attribute__((address_space(3))) int lds_int;
    lds_int *const s_cnt = (lds_int *)(sm + DIAG4_LDS - 2);
    if (tid == 0) *s_cnt = 0;   // ordered before every arrival by the first B1
    auto tile_waves_meet = [&](int target) {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // this wave's -X tiles are in LDS
        if (lane == 0) __hip_atomic_fetch_add(s_cnt, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        while (__hip_atomic_load(s_cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) < target) __builtin_amdgcn_s_sleep(1);
        asm volatile("" ::: "memory");
    };
    d4 XA[8], XB[8], XC[8];
    if (rc == 0) {  // block-row 0 hands tile (0, 0) to the factor wave in matrix order
#pragma unroll
        for (int i = 0; i < 4; ++i) s_d16[0][lr][lq + 4 * i] = TC[0][i];
    }
    int last = -1;  // last step whose non-critical solves and stores are still due
#pragma unroll
    for (int kb = 0; kb < 8; ++kb) {
        if (!FULL && kb >= nblk) break;  // workgroup-uniform
        GPMI_LDS_BARRIER();  // B1: diagonal tile kb is in s_d16[kb & 1] (factor16(kb) starts)
        if (kb > 0) {
            // the rest of step kb - 1: its other rows' solves (row kb was solved before B1) ...
            if (ra != kb) { GPMI_SOLVE_ROW(TA, 8, ra, XA[kb - 1], kb - 1) }
            if (rb != kb) { GPMI_SOLVE_ROW(TB, 5, rb, XB[kb - 1], kb - 1) }
            if (rc != kb) { GPMI_SOLVE_ROW(TC, 2, rc, XC[kb - 1], kb - 1) }
            tile_waves_meet(3 * kb);   // ... every row's -X tile of step kb - 1 is published ...
            GPMI_STORE_STEP(TA, 8, ra, kb - 1, pra)
            GPMI_STORE_STEP(TB, 5, rb, kb - 1, prb)
            GPMI_STORE_STEP(TC, 2, rc, kb - 1, prc)
            // ... and REST: tiles jb >= kb of the rows below, except tile (kb, kb) (updated EARLY)
            if (ra >= kb && GPMI_ACT(ra)) { GPMI_UPDATE_REST(TA, 8, ra, XA[kb - 1]) }
            if (rb >= kb && GPMI_ACT(rb)) { GPMI_UPDATE_REST(TB, 5, rb, XB[kb - 1]) }
            if (rc >= kb && GPMI_ACT(rc)) { GPMI_UPDATE_REST(TC, 2, rc, XC[kb - 1]) }
        }
        GPMI_LDS_BARRIER();  // B2: factor16(kb) done: L16 in s_d16[kb & 1], its inverse in s_inv[kb]
        if (kb < 7 && GPMI_ACT(kb + 1)) {     // the critical row kb + 1: solve, EARLY update of the next diagonal tile, hand-over
            if (ra == kb + 1) { GPMI_SOLVE_ROW(TA, 8, ra, XA[kb], kb) GPMI_UPDATE_EARLY(TA, 8, ra, XA[kb]) }
            else if (rb == kb + 1) { GPMI_SOLVE_ROW(TB, 5, rb, XB[kb], kb) GPMI_UPDATE_EARLY(TB, 5, rb, XB[kb]) }
            else if (rc == kb + 1) { GPMI_SOLVE_ROW(TC, 2, rc, XC[kb], kb) GPMI_UPDATE_EARLY(TC, 2, rc, XC[kb]) }
        }
        last = kb;
    }
#undef GPMI_UPDATE_EARLY
#undef GPMI_UPDATE_REST
    GPMI_BSTAMP(b2)
    // the last step: its diagonal tile back from the factor wave (rows below it are padding: nothing to solve), its stores
    // (compile-time step index: one copy per possible last step of a ragged block)
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        if (k == last) {
            if (ra == k) { GPMI_SOLVE_ROW(TA, 8, ra, XA[k], k) }
            if (rb == k) { GPMI_SOLVE_ROW(TB, 5, rb, XB[k], k) }
            if (rc == k) { GPMI_SOLVE_ROW(TC, 2, rc, XC[k], k) }
            GPMI_STORE_STEP(TA, 8, ra, k, pra)
            GPMI_STORE_STEP(TB, 5, rb, k, prb)
            GPMI_STORE_STEP(TC, 2, rc, k, prc)
        }
    }
#ifdef GPMI_PROBES
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (w == 0 && lane == 0) {
        GPMI_BSTAMP(b3)
        GPMI_BADD(0, b1 - b0)
        GPMI_BADD(1, b2 - b1)
        GPMI_BADD(2, b3 - b2)
        GPMI_BADD(5, 1)
    }
#endif
#undef GPMI_CL
#undef GPMI_ACT
#undef GPMI_LOAD_TILE
#undef GPMI_SOLVE_ROW
#undef GPMI_STORE_STEP
#undef GPMI_LDS_BARRIER
}

// ---------------------------------------------------------------------------
// Panel solve: rows [row0, M) of the nb_act columns starting at Acol.
// X L11^T = A21 by block forward substitution over the 8 block columns; each
// wave carries its 16 rows through all steps in registers.
// ---------------------------------------------------------------------------
// FULL: all 64 rows of the workgroup and all 128 columns exist -- unconditional, batched loads and
// stores from one running column pointer (the guarded form predicates and branches per element)
// kb0 (wave-uniform): the strip's columns left of block kb0 are zero (rows of the identity / of an upper-triangular
// operand): those block steps produce zeros and are skipped
template <bool FULL>
__device__ __forceinline__ void trsm_panel_body(const double *__restrict__ s_F, double *__restrict__ Acol, size_t lda,
                                                int r, bool rok, int nb_act, int tid = (int)threadIdx.x, int kb0 = 0)
{
    const int lane = tid & 63;
    const int lq = lane >> 4;
    const int nblk = FULL ? 8 : (nb_act + 15) >> 4;
    d4 T[8];
    if constexpr (FULL) {
        const double *p = Acol + (size_t)r + (size_t)lq * lda;
#pragma unroll
        for (int jb = 0; jb < 8; ++jb)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                T[jb][i] = *p;
                p += 4 * lda;
            }
    } else {
#pragma unroll
        for (int jb = 0; jb < 8; ++jb) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int col = jb * 16 + lq + 4 * i;
                T[jb][i] = (rok && col < nb_act) ? Acol[(size_t)r + (size_t)col * lda] : 0.0;
            }
        }
    }
    __syncthreads();  // packed factors are in s_F

#pragma unroll
    for (int kb = 0; kb < 8; ++kb) {
        if (kb >= kb0 && kb < nblk) {
            d4 acc = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int kg = 0; kg < 4; ++kg) acc = mfma(s_F[fp_inv(kb) * 256 + kg * 64 + lane], T[kb][kg], acc);
            T[kb] = acc;
#pragma unroll
            for (int jb = kb + 1; jb < 8; ++jb) {
                if (jb < nblk) {
#pragma unroll
                    for (int kg = 0; kg < 4; ++kg)
                        T[jb] = mfma(s_F[fp_l(jb, kb) * 256 + kg * 64 + lane], T[kb][kg], T[jb]);
                }
            }
        }
    }

    if constexpr (FULL) {
        double *p = Acol + (size_t)r + (size_t)lq * lda;
#pragma unroll
        for (int jb = 0; jb < 8; ++jb)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                *p = T[jb][i];
                p += 4 * lda;
            }
    } else {
#pragma unroll
        for (int jb = 0; jb < 8; ++jb) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int col = jb * 16 + lq + 4 * i;
                if (rok && col < nb_act) Acol[(size_t)r + (size_t)col * lda] = T[jb][i];
            }
        }
    }
}

// ---------------------------------------------------------------------------
// GEMM NT on 128x128 tiles.  A: M x K, B: N x K (both with the tile index
// contiguous), C: M x N.  MODE 0: C -= A B^T; 1: same, A == B panel, lower
// tiles only (SYRK); 2: C = A B^T.
// LDS image per stage and operand: [16 k][144] doubles -- each k-row is one
// 1-KiB global_load_lds write; the 128-B row pad puts k and k+1 on opposite
// halves of the 64 banks so the ds_read_b64 fragment reads are conflict-free.
// ---------------------------------------------------------------------------
constexpr int GP = 144;  // GT = 128 and GK = 16 are syrk_walk.h's
// Pair-row layout (PAIR, the blocked update kernels): a lane owns TWO ADJACENT operand rows per pair of MFMA tiles -- inside
// the wave's 64 rows tile t, lane row lr is row (t >> 1) * 32 + 2 * lr + (t & 1) instead of t * 16 + lr -- so that the
// fragments of tiles t, t + 1 (t even) are 16 contiguous bytes of a k-row (one ds_read_b128) and acc[tn][tm][i],
// acc[tn][tm + 1][i] are rows r, r + 1 of one column of C (one 16-byte access).  Which row a lane owns inside an MFMA tile is
// a labelling: every C element sums the same k-terms in the same order.  The image is the same buffer at a k-row pitch of
// GPP doubles: ds_read_b128 is served in lane groups that mix two k-rows (two lq), conflict-free only at a pitch that is
// a multiple of 256 B.
constexpr int GPP = 128;
typedef double d2 __attribute__((ext_vector_type(2)));
// Two adjacent rows of C as ONE 16-byte access.  A global-memory access of any width needs dword alignment only, so the
// pair is typed with the alignment of its elements: a factorisation in place at an odd offset, or with an odd leading
// dimension, takes the same instructions as an aligned one.
typedef d2 d2c __attribute__((aligned(8)));
__device__ __forceinline__ d2 ld_c2(const double *p, bool nt)
{
    return nt ? __builtin_nontemporal_load((const d2c *)p) : *(const d2c *)p;
}
__device__ __forceinline__ void st_c2(double *p, d2 v, bool nt)
{
    if (nt) __builtin_nontemporal_store((d2c)v, (d2c *)p);
    else *(d2c *)p = v;
}

// One 128 x 128 output tile (ti, tj); smem is the workgroup's staging buffer (free on entry:
// every wave has finished reading it).
// MODE 3: the product A B^T is not stored, its elements are consumed where they are (the accumulators never leave their
// registers; C is unused): epi.row(tm, m, ok) announces the lane's four rows, then per column epi.col(n, ok) and
// epi.elem(v, tm) for its four elements -- so that the consumer loads what depends on a row or a column once.
struct NoEpi {
    __device__ void row(int, int, bool) const {}
    __device__ void col(int, bool) const {}
    __device__ void elem(double, int) const {}
};
template <class R, class C, class E>
struct Epi3 {
    R row;
    C col;
    E elem;
};
template <class R, class C, class E>
__device__ __forceinline__ Epi3<R, C, E> make_epi3(R r, C c, E e)
{
    return Epi3<R, C, E>{r, c, e};
}
template <int MODE, bool WHOLE, bool PAIR = false, class EPI = NoEpi>
__device__ __forceinline__ void gemm_tile_k(double (&smem)[2][2][GK][GP], const double *__restrict__ A, size_t lda,
                                            const double *__restrict__ B, size_t ldb, double *__restrict__ C,
                                            size_t ldc, int M, int N, int K, int ti, int tj, int dbg, int tid, EPI &&epi = EPI{})
{
    static_assert(!PAIR || MODE == 0 || MODE == 1, "the pair-row layout is the update kernels'");
    static_assert(2 * 2 * GK * GPP <= 2 * 2 * GK * GP, "the pair-row image lies inside the staging buffer");
    const int m0 = ti * GT, n0 = tj * GT;
    if (MODE == 1 && n0 >= N) return;
    const int lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lr = lane & 15, lq = lane >> 4;
    const int wm = w & 1, wn = w >> 1;

    // staging: waves 0,1 stream the A tile (m index), waves 2,3 the B tile (n index); 8 k-rows each
    const int op = w >> 1;
    const double *gsrc = (op ? B + n0 : A + m0) + 2 * lane;
    const size_t gld = op ? ldb : lda;
    const int krow0 = (w & 1) * 8;

    d4 acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = d4{0.0, 0.0, 0.0, 0.0};

    const int nk = (K + GK - 1) / GK;
    // PAIR: k-row kr of operand o in a stage -- where its 1-KiB DMA lands and where the lane's 16-byte pairs are read
    auto pair_row = [&](int stage, int o, int kr) { return &smem[0][0][0][0] + (size_t)((stage * 2 + o) * GK + kr) * GPP; };
    auto ldpair = [&](int st, int o, int kr, int t, double (&f)[4]) {  // tiles t, t + 1 (t even) of operand o
        const d2 v = *(const d2 *)(pair_row(st, o, kr) + (o ? wn : wm) * 64 + (t >> 1) * 32 + 2 * lr);
        f[t] = v.x;
        f[t + 1] = v.y;
    };
    auto issue = [&](int stage, int k0) {
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int kr = krow0 + q;
            int kc = k0 + kr;
            kc = kc < K ? kc : K - 1;  // clamp: never read a column past the operand
            __builtin_amdgcn_global_load_lds(
                (const __attribute__((address_space(1))) void *)(gsrc + (size_t)kc * gld),
                (__attribute__((address_space(3))) void *)(PAIR ? pair_row(stage, op, kr) : &smem[stage][op][kr][0]), 16, 0, 0);
        }
    };
    // Fragments of sub-step kk+1 are requested before the 16 MFMAs of sub-step kk are issued
    // (two register sets), so the LDS latency sits under ~1k cycles of matrix work.  MASK
    // (zeroing of columns past K) is compiled only into the last, possibly partial, k-step:
    // a select on a just-loaded fragment forces the wait in front of the MFMAs.
    auto ldfrag = [&](auto mk, int st, int kk, int klim, double (&af)[4], double (&bf)[4]) {
        constexpr bool MASK = decltype(mk)::value != 0;
        const int kr = kk * 4 + lq;
        if constexpr (PAIR) {
            ldpair(st, 1, kr, 0, af);
            ldpair(st, 1, kr, 2, af);
            ldpair(st, 0, kr, 0, bf);
            ldpair(st, 0, kr, 2, bf);
        } else {
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                af[t] = smem[st][1][kr][wn * 64 + t * 16 + lr];
                bf[t] = smem[st][0][kr][wm * 64 + t * 16 + lr];
            }
        }
        if constexpr (MASK) {
            const bool kv = kr < klim;
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                af[t] = kv ? af[t] : 0.0;
                bf[t] = kv ? bf[t] : 0.0;
            }
        }
    };
    auto mm16 = [&](const double (&af)[4], const double (&bf)[4]) {
#pragma unroll
        for (int tn = 0; tn < 4; ++tn)
#pragma unroll
            for (int tm = 0; tm < 4; ++tm) acc[tn][tm] = mfma(af[tn], bf[tm], acc[tn][tm]);
    };
    // mid(): issued between the first fragment reads and the first MFMAs (the DMA of the next stage:
    // its instructions then run under the LDS latency instead of in front of it)
    auto compute = [&](auto mk, int st, int klim, auto &&mid) {
        double a0[4], b0[4], a1[4], b1[4];
        ldfrag(mk, st, 0, klim, a0, b0);
        ldfrag(mk, st, 1, klim, a1, b1);
        __builtin_amdgcn_sched_barrier(0);
        mid();
        __builtin_amdgcn_sched_barrier(0);
        mm16(a0, b0);
        __builtin_amdgcn_sched_barrier(0);
        ldfrag(mk, st, 2, klim, a0, b0);
        __builtin_amdgcn_sched_barrier(0);
        mm16(a1, b1);
        __builtin_amdgcn_sched_barrier(0);
        ldfrag(mk, st, 3, klim, a1, b1);
        __builtin_amdgcn_sched_barrier(0);
        mm16(a0, b0);
        mm16(a1, b1);
    };

    if constexpr (WHOLE) {
        const double *g0 = gsrc + (size_t)krow0 * gld;
#pragma unroll
        for (int q = 0; q < 8; ++q)  // stage 0, same lean addressing as the loop
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(g0 + (size_t)q * gld),
                                             (__attribute__((address_space(3))) void *)(PAIR ? pair_row(0, op, krow0 + q) : &smem[0][op][krow0 + q][0]), 16, 0, 0);
    } else {
        issue(0, 0);
    }
    double a0[4], b0[4];  // whole-k-step form: the fragments of sub-step 0 cross the k-step boundary
    if constexpr (WHOLE) {
        // Whole k-steps only (every launch of a factorisation whose order is a multiple of 16): no
        // clamp, and the eight row addresses of a stage are one running per-lane pointer plus
        // loop-invariant uniform offsets -- one VALU add per DMA instead of the ~12 scalar
        // instructions (min, 64-bit multiply, ...) of the general form.
        // The k-step boundary is software-pipelined (round 3): the barrier that publishes stage t + 1 sits BEFORE the
        // last 16 MFMAs of step t, and the DMA of step t + 2 and the first fragment reads of step t + 1 are issued
        // between those MFMAs -- so what a k-step exposes is the barrier itself, not barrier + DMA issue + LDS latency
        // in front of its first MFMA (4970 cycles per 4096 of MFMA issue for a workgroup alone on a CU before).
        // Stage t & 1 is free for the DMA of step t + 2 at that barrier: every wave has its last fragments of step t
        // in registers (lgkmcnt(0) in front of the barrier).
        const double *gp = gsrc + (size_t)krow0 * gld;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (nk > 1 && !(dbg & 2)) {
            gp += (size_t)GK * gld;
            asm volatile("" : "+v"(gp));
#pragma unroll
            for (int q = 0; q < 8; ++q)
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(gp + (size_t)q * gld),
                                                 (__attribute__((address_space(3))) void *)(PAIR ? pair_row(1, op, krow0 + q) : &smem[1][op][krow0 + q][0]), 16, 0, 0);
        }
        ldfrag(ic<0>{}, 0, 0, GK, a0, b0);
        // one k-step that has a successor; DMA: the step after that exists and is requested here
        auto kstep = [&](auto dma, int st) {
            constexpr bool DMA = decltype(dma)::value != 0;
            double a1[4], b1[4];
            // the first reads of a1, b1 go out BEHIND the first four MFMAs: the wait in front of those then covers a0, b0
            // only (issued a quarter of a k-step ago), not an LDS round trip
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int tm = 0; tm < 4; ++tm) acc[0][tm] = mfma(a0[0], b0[tm], acc[0][tm]);
            __builtin_amdgcn_sched_barrier(0);
            ldfrag(ic<0>{}, st, 1, GK, a1, b1);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int tn = 1; tn < 4; ++tn)
#pragma unroll
                for (int tm = 0; tm < 4; ++tm) acc[tn][tm] = mfma(a0[tn], b0[tm], acc[tn][tm]);
            __builtin_amdgcn_sched_barrier(0);
            ldfrag(ic<0>{}, st, 2, GK, a0, b0);
            __builtin_amdgcn_sched_barrier(0);
            mm16(a1, b1);
            __builtin_amdgcn_sched_barrier(0);
            ldfrag(ic<0>{}, st, 3, GK, a1, b1);
            __builtin_amdgcn_sched_barrier(0);
            mm16(a0, b0);
            __builtin_amdgcn_sched_barrier(0);
            asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
            // keep ONE running per-lane pointer (opaque to the optimiser, which otherwise turns the
            // eight invariant offsets into eight running scalar pointers: 16 SALU per k-step)
            gp += (size_t)GK * gld;
            asm volatile("" : "+v"(gp));
#pragma unroll
            for (int tn = 0; tn < 4; ++tn) {
#pragma unroll
                for (int tm = 0; tm < 4; ++tm) acc[tn][tm] = mfma(a1[tn], b1[tm], acc[tn][tm]);
                __builtin_amdgcn_sched_barrier(0);
                if constexpr (PAIR) {  // one 16-byte read behind each four MFMAs: a0 pair 0, b0 pair 0, a0 pair 1, b0 pair 1
                    if (tn & 1) ldpair(st ^ 1, 0, lq, tn & 2, b0);
                    else ldpair(st ^ 1, 1, lq, tn & 2, a0);
                } else {
                    a0[tn] = smem[st ^ 1][1][lq][wn * 64 + tn * 16 + lr];
                    b0[tn] = smem[st ^ 1][0][lq][wm * 64 + tn * 16 + lr];
                }
                if constexpr (DMA) if (tn < 2) {  // all eight requests behind the first eight MFMAs: they have until the next barrier
#pragma unroll
                    for (int q = 4 * tn; q < 4 * tn + 4; ++q)
                        __builtin_amdgcn_global_load_lds(
                            (const __attribute__((address_space(1))) void *)(gp + (size_t)q * gld),
                            (__attribute__((address_space(3))) void *)(PAIR ? pair_row(st, op, krow0 + q) : &smem[st][op][krow0 + q][0]), 16, 0, 0);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        };
        if (dbg & 2) {
#pragma unroll 1
            for (int kt = 0; kt < nk - 1; ++kt) kstep(ic<0>{}, kt & 1);
        } else {
#pragma unroll 1
            for (int kt = 0; kt < nk - 2; ++kt) kstep(ic<1>{}, kt & 1);
            if (nk > 1) kstep(ic<0>{}, nk & 1);  // step nk - 2: nothing left to request
        }
    } else {
#pragma unroll 1
        for (int kt = 0; kt < nk - 1; ++kt) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            if (!(dbg & 2)) issue((kt + 1) & 1, (kt + 1) * GK);
            compute(ic<0>{}, kt & 1, GK, []() {});
        }
    }

    // Last k-step peeled.  For a tile wholly inside the matrix the first half of the C tile
    // (32 loads per lane, uniform offsets from one base) is issued under that step -- the
    // staging loads are all retired by then -- and the second half right after the first
    // half's stores: one memory round trip is exposed per tile instead of four.  For SYRK the
    // diagonal tiles are computed in full (their strictly-upper outputs land in the unused
    // upper triangle of the workspace).
    const bool interior = (m0 + GT <= M) && (n0 + GT <= N);
    double *const cbase = C + (size_t)(m0 + wm * 64 + lr) + (size_t)(n0 + wn * 64 + lq) * ldc;
    double ch[2][4][4];
    const bool cnt = (dbg & 8) != 0;
    if constexpr (!WHOLE) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }
    if (!PAIR && MODE != 2 && MODE != 3 && interior) {
#pragma unroll
        for (int tn = 0; tn < 2; ++tn)
#pragma unroll
            for (int tm = 0; tm < 4; ++tm)
#pragma unroll
                for (int i = 0; i < 4; ++i) ch[tn][tm][i] = ld_c(cbase + tm * 16 + (size_t)(tn * 16 + 4 * i) * ldc, cnt);
    }
    // PAIR: the lane's rows prow(tm), prow(tm + 1) = prow(tm) + 1 (tm even) and columns pcol(tn, i); half h of the C tile is
    // tn = 2 h, 2 h + 1: 16 accesses of 16 bytes from one base
    auto prow = [&](int tm) { return m0 + wm * 64 + (tm >> 1) * 32 + 2 * lr + (tm & 1); };
    auto pcol = [&](int tn, int i) { return n0 + wn * 64 + (tn >> 1) * 32 + 2 * (lq + 4 * i) + (tn & 1); };
    double *const cpair = PAIR ? C + (size_t)prow(0) + (size_t)pcol(0, 0) * ldc : nullptr;
    d2 cp[2][2][4];  // [tn & 1][tm >> 1][i]
    auto cp_at = [&](int tn, int p, int i) { return cpair + p * 32 + (size_t)((tn >> 1) * 32 + 8 * i + (tn & 1)) * ldc; };
    auto cp_load = [&](int h) {
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int p = 0; p < 2; ++p)
#pragma unroll
                for (int i = 0; i < 4; ++i) cp[t][p][i] = ld_c2(cp_at(2 * h + t, p, i), cnt);
    };
    auto cp_store = [&](int h) {
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int p = 0; p < 2; ++p)
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    st_c2(cp_at(2 * h + t, p, i),
                          d2{cp[t][p][i].x - acc[2 * h + t][2 * p][i], cp[t][p][i].y - acc[2 * h + t][2 * p + 1][i]}, cnt);
    };
    if constexpr (PAIR) {
        if (interior) cp_load(0);
    }
    if constexpr (WHOLE) {  // the fragments of sub-step 0 of the last stage are in registers
        const int st = (nk - 1) & 1;
        double a1[4], b1[4];
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int tm = 0; tm < 4; ++tm) acc[0][tm] = mfma(a0[0], b0[tm], acc[0][tm]);
        __builtin_amdgcn_sched_barrier(0);
        ldfrag(ic<0>{}, st, 1, GK, a1, b1);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int tn = 1; tn < 4; ++tn)
#pragma unroll
            for (int tm = 0; tm < 4; ++tm) acc[tn][tm] = mfma(a0[tn], b0[tm], acc[tn][tm]);
        __builtin_amdgcn_sched_barrier(0);
        ldfrag(ic<0>{}, st, 2, GK, a0, b0);
        __builtin_amdgcn_sched_barrier(0);
        mm16(a1, b1);
        __builtin_amdgcn_sched_barrier(0);
        ldfrag(ic<0>{}, st, 3, GK, a1, b1);
        __builtin_amdgcn_sched_barrier(0);
        mm16(a0, b0);
        mm16(a1, b1);
    } else {
        compute(ic<1>{}, (nk - 1) & 1, K - (nk - 1) * GK, []() {});
    }
    if (dbg & 1) {
        double sacc = 0.0;
#pragma unroll
        for (int tn = 0; tn < 4; ++tn)
#pragma unroll
            for (int tm = 0; tm < 4; ++tm)
#pragma unroll
                for (int i = 0; i < 4; ++i) sacc += acc[tn][tm][i];
        if (sacc == 1.2345e300) cbase[0] = sacc;
        return;
    }
    if constexpr (MODE == 3) {
#pragma unroll
        for (int tm = 0; tm < 4; ++tm) {
            const int m = m0 + wm * 64 + tm * 16 + lr;
            epi.row(tm, m, m < M);
        }
#pragma unroll
        for (int tn = 0; tn < 4; ++tn)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int n = n0 + wn * 64 + tn * 16 + lq + 4 * i;
                epi.col(n, n < N);
#pragma unroll
                for (int tm = 0; tm < 4; ++tm) epi.elem(acc[tn][tm][i], tm);
            }
        return;
    }
    if constexpr (PAIR) {
        if (interior) {
            cp_store(0);
            cp_load(1);
            cp_store(1);
            return;
        }
        // edge tile, as below with the lane's pair-row indices
#pragma unroll
        for (int tn = 0; tn < 4; ++tn) {
            double ce[4][4];
#pragma unroll
            for (int tm = 0; tm < 4; ++tm)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    int n = pcol(tn, i), m = prow(tm);
                    n = n < N ? n : N - 1;
                    m = m < M ? m : M - 1;
                    ce[tm][i] = C[(size_t)m + (size_t)n * ldc];
                }
#pragma unroll
            for (int tm = 0; tm < 4; ++tm)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int n = pcol(tn, i), m = prow(tm);
                    if (m < M && n < N && (MODE != 1 || n <= m)) C[(size_t)m + (size_t)n * ldc] = ce[tm][i] - acc[tn][tm][i];
                }
        }
        return;
    }
    if (interior) {
#pragma unroll
        for (int tn = 0; tn < 2; ++tn)
#pragma unroll
            for (int tm = 0; tm < 4; ++tm)
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    st_c(cbase + tm * 16 + (size_t)(tn * 16 + 4 * i) * ldc,
                         (MODE == 2) ? acc[tn][tm][i] : ch[tn][tm][i] - acc[tn][tm][i], cnt);
        if (MODE != 2) {
#pragma unroll
            for (int tn = 0; tn < 2; ++tn)
#pragma unroll
                for (int tm = 0; tm < 4; ++tm)
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        ch[tn][tm][i] = ld_c(cbase + tm * 16 + (size_t)((tn + 2) * 16 + 4 * i) * ldc, cnt);
        }
#pragma unroll
        for (int tn = 0; tn < 2; ++tn)
#pragma unroll
            for (int tm = 0; tm < 4; ++tm)
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    st_c(cbase + tm * 16 + (size_t)((tn + 2) * 16 + 4 * i) * ldc,
                         (MODE == 2) ? acc[tn + 2][tm][i] : ch[tn][tm][i] - acc[tn + 2][tm][i], cnt);
        return;
    }

    // edge tile: per tn, 16 loads from clamped (always valid) addresses, then guarded stores
#pragma unroll
    for (int tn = 0; tn < 4; ++tn) {
        double ce[4][4];
#pragma unroll
        for (int tm = 0; tm < 4; ++tm)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                int n = n0 + wn * 64 + tn * 16 + lq + 4 * i, m = m0 + wm * 64 + tm * 16 + lr;
                n = n < N ? n : N - 1;
                m = m < M ? m : M - 1;
                if (MODE != 2) ce[tm][i] = C[(size_t)m + (size_t)n * ldc];
            }
#pragma unroll
        for (int tm = 0; tm < 4; ++tm)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int n = n0 + wn * 64 + tn * 16 + lq + 4 * i, m = m0 + wm * 64 + tm * 16 + lr;
                if (m < M && n < N && (MODE != 1 || n <= m))
                    C[(size_t)m + (size_t)n * ldc] = (MODE == 2) ? acc[tn][tm][i] : ce[tm][i] - acc[tn][tm][i];
            }
    }
}


// Whole k-steps (every launch of a factorisation whose order is a multiple of 16) take the software-pipelined form;
// the two forms are separate instantiations so that neither's live ranges weigh on the other's register allocation.
template <int MODE, bool PAIR = false, class EPI = NoEpi>
__device__ __forceinline__ void gemm_tile(double (&smem)[2][2][GK][GP], const double *__restrict__ A, size_t lda,
                                          const double *__restrict__ B, size_t ldb, double *__restrict__ C,
                                          size_t ldc, int M, int N, int K, int ti, int tj, int dbg, int tid, EPI &&epi = EPI{})
{
    if (K % GK == 0 && !(dbg & 16)) gemm_tile_k<MODE, true, PAIR>(smem, A, lda, B, ldb, C, ldc, M, N, K, ti, tj, dbg, tid, epi);  // workgroup-uniform
    else gemm_tile_k<MODE, false, PAIR>(smem, A, lda, B, ldb, C, ldc, M, N, K, ti, tj, dbg, tid, epi);
}


// 64 x 64 tile of C -= A B^T, LDS-staged: the quadrant kernel of the SYRK tail split.  Four waves
// x (2 x 2 MFMA tiles), k-step 16, two LDS stages filled through registers (16-B global loads,
// ds_write_b128; row pad 16 doubles: k and k + 1 on opposite bank halves as in the big tile).
// A, B point at the quadrant's first operand rows; mv / nv valid rows from there (clamped loads,
// dropped outputs).  K % 16 == 0.
constexpr int QP = 80;  // padded row of the quadrant's LDS image
__device__ __forceinline__ void gemm_quad64(double *__restrict__ sm, const double *__restrict__ A, size_t lda,
                                            const double *__restrict__ B, size_t ldb, double *__restrict__ C,
                                            size_t ldc, int K, int mv, int nv, int tid)
{
    double (*q)[2][GK][QP] = reinterpret_cast<double (*)[2][GK][QP]>(sm);  // [stage][op][k][row]
    const int lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lr = lane & 15, lq = lane >> 4;
    const int mb = (w & 1) * 32, nb = (w >> 1) * 32;
    // staging: thread handles the row pair r2 of k-rows kr and kr + 8 of both operands
    const int r2 = tid & 31, kr = tid >> 5;
    const bool fast = (mv >= 64) && (nv >= 64);
    int ra0 = 2 * r2, ra1 = 2 * r2 + 1, rb0 = ra0, rb1 = ra1;
    ra0 = ra0 < mv ? ra0 : mv - 1;
    ra1 = ra1 < mv ? ra1 : mv - 1;
    rb0 = rb0 < nv ? rb0 : nv - 1;
    rb1 = rb1 < nv ? rb1 : nv - 1;
    double2 va[2], vb[2];
    auto gload = [&](int k0) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const size_t ca = (size_t)(k0 + kr + 8 * j) * lda, cb = (size_t)(k0 + kr + 8 * j) * ldb;
            if (fast) {
                va[j] = *reinterpret_cast<const double2 *>(A + 2 * r2 + ca);
                vb[j] = *reinterpret_cast<const double2 *>(B + 2 * r2 + cb);
            } else {
                va[j] = make_double2(A[ra0 + ca], A[ra1 + ca]);
                vb[j] = make_double2(B[rb0 + cb], B[rb1 + cb]);
            }
        }
    };
    auto swrite = [&](int st) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            *reinterpret_cast<double2 *>(&q[st][0][kr + 8 * j][2 * r2]) = va[j];
            *reinterpret_cast<double2 *>(&q[st][1][kr + 8 * j][2 * r2]) = vb[j];
        }
    };
    d4 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[a][b] = d4{0.0, 0.0, 0.0, 0.0};
    const int nk = K / GK;
    gload(0);
    swrite(0);
    __syncthreads();
#pragma unroll 1
    for (int kt = 0; kt < nk; ++kt) {
        const int st = kt & 1;
        if (kt + 1 < nk) gload((kt + 1) * GK);
        if (mb < mv && nb < nv) {  // wave-uniform: a wave whose block lies outside the matrix only stages
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                double af[2], bf[2];
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    af[t] = q[st][1][kk * 4 + lq][nb + t * 16 + lr];
                    bf[t] = q[st][0][kk * 4 + lq][mb + t * 16 + lr];
                }
#pragma unroll
                for (int tn = 0; tn < 2; ++tn)
#pragma unroll
                    for (int tm = 0; tm < 2; ++tm)
                        if (mb + tm * 16 < mv && nb + tn * 16 < nv) acc[tn][tm] = mfma(af[tn], bf[tm], acc[tn][tm]);
            }
        }
        if (kt + 1 < nk) swrite(st ^ 1);
        __syncthreads();
    }
#pragma unroll
    for (int tn = 0; tn < 2; ++tn)
#pragma unroll
        for (int tm = 0; tm < 2; ++tm)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int m = mb + tm * 16 + lr, n = nb + tn * 16 + lq + 4 * i;
                if (m < mv && n < nv) {
                    double *c = C + (size_t)m + (size_t)n * ldc;
                    *c = *c - acc[tn][tm][i];
                }
            }
}

constexpr int FIN_SLICE = 256;  // slice of the diagonal one workgroup of k_logml_partial reduces

}  // namespace
