// The trailing update's tile walks and launch plan: integer arithmetic on (M, N, K, slots, options).  The walks are what
// k_gemm_nt<1> (chol_kernels.hip) decodes its block index with; the plan is what launch_syrk_lower launches, and a host program
// can sweep it (tests/syrk_plan_host.cpp).  Nothing here needs the HIP runtime: a plain C++ compiler takes this header as it is.
#pragma once
#include <math.h>

#ifndef __HIPCC__
#ifndef __host__
#define __host__
#endif
#ifndef __device__
#define __device__
#endif
#ifndef __forceinline__
#define __forceinline__ inline __attribute__((always_inline))
#endif
#endif

namespace {

constexpr int GT = 128, GK = 16;  // tile order of the update kernels, k-rows per LDS stage
constexpr int SUBWG = 9;  // workgroups (x 4 waves = 36 sub-tiles of 16 x 16) of the sub-tiled diagonal tile of a fused launch

// SYRK tile order 0: block b is tile b of the row-major walk of the lower triangle.
// TN < T: the lower TRAPEZOID of a T x TN tile grid (a trailing matrix with more rows than columns,
// e.g. the augmented row): the TN x TN triangle first, then the rows below it.
__host__ __device__ __forceinline__ bool syrk_tile(int b, int T, int TN, int order, int &ti, int &tj)
{
    if (order == 0) {  // plain row-major walk of the lower triangle / trapezoid
        const int tri = TN * (TN + 1) / 2;
        if (b >= tri) {
            const int q = b - tri;
            ti = TN + q / TN;
            tj = q % TN;
            return ti < T;
        }
        int i = (int)((sqrt(8.0 * (double)b + 1.0) - 1.0) * 0.5);
        while ((i + 1) * (i + 2) / 2 <= b) ++i;
        while (i * (i + 1) / 2 > b) --i;
        ti = i;
        tj = b - i * (i + 1) / 2;
        return ti < T;
    }
    return false;  // walk 2 has its own enumeration (syrk_tile_bands); no other walk exists
}
__host__ inline int syrk_grid(int T, int TN) { return TN * (TN + 1) / 2 + (T - TN) * TN; }  // tiles of the triangle / trapezoid

// XCD-partitioned band walk (order 2) of the lower triangle / trapezoid, WITHOUT a padded grid: the valid tiles are
// enumerated band by band (8 tile rows), inside a band column by column -- 64 consecutive tiles are an 8 x 8 patch --
// and workgroup b takes canonical tile (b % 8) S + b / 8, S = ceil(ntiles / 8): the workgroups the dispatcher deals to
// one XCD (observed: b % 8; speed only, any placement is correct) walk ONE contiguous eighth of that order.  The 64
// tiles resident on an XCD at a time then share 8 row blocks (for a whole band) and 8 column blocks of the panel
// through that XCD's L2 instead of ~5 + 15 that change every round.  Every XCD gets the same number of tiles, so the
// launch ends as evenly as the row-major walk; the last partial round of EACH XCD is what the tail split cuts into
// quadrants, and a thin last tile row (the augmented row) is multiplied as quadrants by its own workgroup.
__host__ __device__ __forceinline__ void syrk_tile_bands(int c, int T, int TN, int &ti, int &tj)
{
    for (int r0 = 0;; r0 += 8) {
        const int R = (T - r0 < 8) ? T - r0 : 8;
        const int cf = r0 < TN ? r0 : TN;                          // columns left of the band's diagonal block: R tiles each
        const int dmax = (TN - r0 < R) ? (TN - r0 > 0 ? TN - r0 : 0) : R;  // columns r0 + d of the diagonal block: rows d .. R - 1
        const int cnt = R * cf + dmax * R - dmax * (dmax - 1) / 2;
        if (c < cnt || R <= 0) {
            if (c < R * cf) {
                tj = c / R;
                ti = r0 + c - tj * R;
                return;
            }
            c -= R * cf;
            int d = 0;
            while (d < dmax - 1 && c >= R - d) {
                c -= R - d;
                ++d;
            }
            tj = r0 + d;
            ti = r0 + d + c;
            return;
        }
        c -= cnt;
    }
}

// Tail split of a SYRK launch: the R < slots tiles of the last, partial round would hold R
// workgroup slots for a whole tile time while the rest of the chip idles.  Each of them is cut
// into its four 64 x 64 quadrants (blocks bfull + 4 t + q), computed by gemm_quad64: independent
// outputs, no exchange between workgroups, the same sums in the same order as timing-independent
// code must have.
struct KSplit {
    int bfull;   // blocks below this index are whole tiles
    int S;       // 4: quadrants; <= 1: no split
};

// ---- the launch plan ---------------------------------------------------------------------------------------------------
// tune.ksplit      quadrant split of the tail-round tiles of a SYRK launch (see KSplit) ...
// tune.ksplit_max  ... when at most this many tiles are left for the last round.  Whole tiles of a round this thin run
// alone on their CUs (~115 us at K = 1024 instead of ~250 us shared); four quadrant workgroups take
// ~75 us as long as they, too, have CUs of their own (4 R <= ~400).  Measured per launch (K = 1024):
// R = 16..92: -0.04 .. -0.065 ms; R = 136..340: +0.03 .. +0.06 ms.
struct SyrkTune {   // the switches of gpmi_tuning the plan reads
    int syrk_order, stagger, fuse_diag, ksplit, ksplit_max;
};
struct SyrkPlan {
    bool launch;       // false: an empty update, nothing to launch
    int grid;          // workgroups
    int order;         // walk (bits 0 .. 7) | 0x100 upper-triangular panel | 0x200 sub-tiled tile (0, 0)
    int stagger;
    KSplit ks;
    bool fuse;         // the launch factors the offered diagonal block at C's origin
    bool multi_round;  // more tiles than workgroup slots: a throughput-bound launch
};

__host__ inline int syrk_slots(int ncu) { return 2 * (ncu > 0 ? ncu : 256); }  // two workgroups of the update kernel per CU

// C(lower) -= P P^T, C: M x N (N < M: lower trapezoid), P: M x K.  slots: syrk_slots() of the CU count the plan is made
// for; diag: a diagonal block at C's origin is offered for fusion (fuse_diag bit 3 is cleared by a caller without a
// counter for the sub-tile blocks); tri: P is upper triangular.
__host__ inline SyrkPlan syrk_plan(int M, int N, int K, int slots, const SyrkTune &tune, int lanes_active, bool diag, int tri)
{
    SyrkPlan p{};
    if (M <= 0 || N <= 0 || K <= 0) return p;
    p.launch = true;
    const int T = (M + GT - 1) / GT;
    if (tri) {  // upper-triangular panel: plain kernel, row-major tiles, zero K-range skipped
        p.grid = syrk_grid(T, T);
        p.order = 0x100;
        return p;
    }
    // N < M: lower trapezoid
    const int TNf = (N + GT - 1) / GT, TN = TNf < T ? TNf : T;
    const int ntiles = syrk_grid(T, TN);
    p.multi_round = ntiles > slots;
    // tile walk: 0 row-major; 2 XCD-partitioned bands (launches of more than one round of tiles: that is where the
    // operand re-reads that miss the XCD L2s come from).
    // Walk 2 is the default for an evaluation that has the chip to itself (N = 16384: L2 hit rate 53 -> 79 %, L2-miss
    // traffic 1.27 -> 0.65 GB per launch, 27.31 -> 27.07 ms); under the grid lanes, where four launches share every
    // XCD, its static per-XCD partition loses 1.6 % (23.09 -> 23.45 ms per point) and the row-major walk stays.
    const int syrk_order = (tune.syrk_order == 2 && !lanes_active && p.multi_round) ? 2 : 0;
    p.stagger = ntiles >= 1024 ? tune.stagger : 0;  // only when every CU holds two workgroups for many rounds
    // only in launches of more than one round of tiles, where workgroup 0's extra 27 us do not
    // lengthen the kernel
    p.fuse = diag && (tune.fuse_diag & 2) && p.multi_round;  // tile (0, 0) is block 0 in walks 0 and 2
    // Single-round launches: the next diagonal block rides along as well, sub-tiled like in the in-block products
    // (fused_subtiles_and_diag) -- its 36 sub-tiles and the block's factorisation (~6 + 21 us) run beside the other
    // tiles instead of in a kernel of their own behind the launch (tune.fuse_diag bit 3).
    p.order = syrk_order;
    if (!p.fuse && diag && (tune.fuse_diag & 8) && syrk_order == 0 && M >= GT && N >= GT && K % 64 == 0) {
        p.fuse = true;
        p.order |= 0x200;
    }
    p.grid = ntiles;
    if (syrk_order == 2) {
        // every XCD walks S tiles on its slots / 8 workgroup slots: its last partial round, when thin, runs as quadrants
        // (quadrant 0 by the tile's own workgroup, 1 .. 3 by workgroups behind the grid)
        const int S = (ntiles + 7) / 8, per = slots / 8;
        const int S_full = (S / per) * per, Rx = S - S_full;
        p.grid = 8 * S;
        if (tune.ksplit && K % GK == 0 && Rx > 0 && 8 * Rx <= tune.ksplit_max) {
            p.ks = KSplit{S_full, 4};
            p.grid += 3 * 8 * Rx;
        }
    } else
    if (tune.ksplit && syrk_order == 0 && K % GK == 0) {
        int first = ntiles;  // first tile computed as quadrants
        const int bfull = (ntiles / slots) * slots, R = ntiles - bfull;
        if (R > 0 && R <= tune.ksplit_max) first = bfull;
        // A last tile row with few valid rows -- the augmented row y^T of the marginal likelihood makes
        // every trailing update end in a row of T tiles with ONE valid row -- costs a whole tile time
        // per tile (2.4 % of all tiles at N = 16384); as quadrants only the MFMA tiles that hold
        // valid rows are multiplied (1/8 of the work).
        const int vlast = M - (T - 1) * GT;
        if (T > 1 && vlast <= 64 && ntiles - TN < first) first = ntiles - TN;  // the last tile row has TN tiles
        if ((p.order & 0x200) && first < 1) first = 1;  // tile 0 belongs to the sub-tile blocks
        if (first < ntiles) {
            p.ks = KSplit{first, 4};
            p.grid = first + 4 * (ntiles - first);
        }
    }
    if (p.order & 0x200) p.grid += SUBWG - 1;
    return p;
}

}  // namespace
