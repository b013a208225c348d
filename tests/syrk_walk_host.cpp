// Host program over gp_amd/csrc/syrk_walk.h, the trailing update's tile walks and launch plan (tests/test_syrk_walk_host.py
// compiles and runs it; it needs no GPU and no HIP header).
//   syrk_walk_host sweep      every combination of the sweep below: the two tile walks enumerate each tile of the lower
//                             triangle / trapezoid exactly once, and the plan keeps the invariants the kernel relies on.
//                             Prints the first violations with their combination and exits 1.
//   syrk_walk_host classify   reads lines "M N K slots syrk_order ksplit ksplit_max fuse_diag lanes_active diag" and prints
//                             the path class of each plan: "walk=W multi=B tail=B thin=B fused=multi|single|none shape=tri|trap"
// k_gemm_nt<1> decodes its block index itself (chol_kernels.hip): which block multiplies which quadrant is not stated in the
// header, so this program does not walk the blocks of a grid.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#include "../gp_amd/csrc/syrk_walk.h"

namespace {

int g_fail = 0;
long g_plans = 0;

struct Combo {
    int M, N, K, slots, lanes, diag;
    SyrkTune t;
};

void fail(const char *what, const Combo &c, const SyrkPlan &p)
{
    if (++g_fail <= 20)
        printf("VIOLATION %s: M=%d N=%d K=%d slots=%d syrk_order=%d ksplit=%d ksplit_max=%d fuse_diag=%d lanes=%d diag=%d -> "
               "grid=%d order=0x%x stagger=%d ks={%d,%d} fuse=%d multi_round=%d\n",
               what, c.M, c.N, c.K, c.slots, c.t.syrk_order, c.t.ksplit, c.t.ksplit_max, c.t.fuse_diag, c.lanes, c.diag, p.grid,
               p.order, p.stagger, p.ks.bfull, p.ks.S, (int)p.fuse, (int)p.multi_round);
}

// both walks are bijections from [0, ntiles) onto the tiles ti >= tj, tj < TN, ti < T; the row-major walk ends there
void check_walks(int T, int TN)
{
    const int nt = syrk_grid(T, TN);
    for (int walk = 0; walk < 2; ++walk) {
        std::vector<int> seen((size_t)T * TN, 0);
        for (int b = 0; b < nt; ++b) {
            int ti = -1, tj = -1;
            bool ok = true;
            if (walk == 0) ok = syrk_tile(b, T, TN, 0, ti, tj);
            else syrk_tile_bands(b, T, TN, ti, tj);
            if (!ok || ti < 0 || ti >= T || tj < 0 || tj >= TN || tj > ti) {
                if (++g_fail <= 20) printf("VIOLATION walk %d: T=%d TN=%d index %d -> tile (%d, %d)\n", walk ? 2 : 0, T, TN, b, ti, tj);
                continue;
            }
            if (++seen[(size_t)ti * TN + tj] != 1 && ++g_fail <= 20)
                printf("VIOLATION walk %d: T=%d TN=%d tile (%d, %d) twice (index %d)\n", walk ? 2 : 0, T, TN, ti, tj, b);
        }
        int ti, tj;
        if (walk == 0 && syrk_tile(nt, T, TN, 0, ti, tj) && ++g_fail <= 20)
            printf("VIOLATION walk 0: T=%d TN=%d index %d past the last tile is taken as (%d, %d)\n", T, TN, nt, ti, tj);
    }
    int ti = -1, tj = -1;
    syrk_tile_bands(0, T, TN, ti, tj);
    if ((ti || tj) && ++g_fail <= 20) printf("VIOLATION walk 2: T=%d TN=%d index 0 is tile (%d, %d)\n", T, TN, ti, tj);
    if ((!syrk_tile(0, T, TN, 0, ti, tj) || ti || tj) && ++g_fail <= 20) printf("VIOLATION walk 0: T=%d TN=%d index 0 is tile (%d, %d)\n", T, TN, ti, tj);
}

struct Class {
    int walk;
    bool multi, tail, thin, trap;
    const char *fused;
};

Class classify(const Combo &c, const SyrkPlan &p)
{
    const int T = (c.M + GT - 1) / GT, TNf = (c.N + GT - 1) / GT, TN = TNf < T ? TNf : T;
    const int nt = syrk_grid(T, TN), vlast = c.M - (T - 1) * GT;
    Class k{};
    k.walk = p.order & 0xff;
    k.multi = p.multi_round;
    k.trap = TN < T;
    const bool thin_row = T > 1 && vlast <= 64 && c.K % GK == 0;  // a last tile row the kernel may take as quadrants
    if (k.walk == 2) {
        k.tail = p.ks.S > 1;       // the last partial round of every XCD as quadrants
        k.thin = thin_row;         // the band walk's blocks decide this themselves
    } else {
        k.thin = thin_row && p.ks.S > 1 && p.ks.bfull <= nt - TN;
        k.tail = p.ks.S > 1 && p.ks.bfull < nt - (k.thin ? TN : 0);  // quadrant tiles in front of the thin row
    }
    k.fused = !p.fuse ? "none" : ((p.order & 0x200) ? "single" : "multi");
    return k;
}

void check_plan(const Combo &c)
{
    const SyrkPlan p = syrk_plan(c.M, c.N, c.K, c.slots, c.t, c.lanes, c.diag != 0, 0);
    ++g_plans;
    const int T = (c.M + GT - 1) / GT, TNf = (c.N + GT - 1) / GT, TN = TNf < T ? TNf : T;
    const int nt = syrk_grid(T, TN), walk = p.order & 0xff;
    if (!p.launch) { fail("a non-empty update is not launched", c, p); return; }
    if (walk != 0 && walk != 2) fail("unknown walk", c, p);
    if (p.order & ~0x2ff) fail("unknown order bits", c, p);
    if (p.multi_round != (nt > c.slots)) fail("multi_round is not ntiles > slots", c, p);
    if (walk == 2 && (!p.multi_round || c.lanes || c.t.syrk_order != 2)) fail("band walk outside a lone multi-round launch", c, p);
    if (p.stagger && nt < 1024) fail("stagger in a short launch", c, p);
    if (p.ks.S > 1 && (c.K % GK || !c.t.ksplit || p.ks.S != 4)) fail("quadrants the quadrant product cannot take", c, p);
    // the grid holds exactly the blocks the kernel decodes: whole tiles, four blocks per quadrant tile (walk 0) or quadrant 0
    // in the tile's own block and three behind the grid (walk 2), the sub-tile blocks in place of tile 0
    const int sub = (p.order & 0x200) ? SUBWG - 1 : 0;
    if (walk == 0) {
        if (p.ks.S > 1) {
            if (p.ks.bfull < 0 || p.ks.bfull >= nt) fail("walk 0: first quadrant tile outside the grid", c, p);
            if (p.grid != p.ks.bfull + 4 * (nt - p.ks.bfull) + sub) fail("walk 0: grid size", c, p);
            const int R = nt % c.slots, vlast = c.M - (T - 1) * GT;
            const bool thin = T > 1 && vlast <= 64;
            int first = (R > 0 && R <= c.t.ksplit_max) ? nt - R : nt;
            if (thin && nt - TN < first) first = nt - TN;
            if (sub && first < 1) first = 1;
            if (p.ks.bfull != first) fail("walk 0: quadrant tiles are not the tail round and the thin last row", c, p);
        } else if (p.grid != nt + sub) fail("walk 0: grid size", c, p);
    } else {
        const int S = (nt + 7) / 8;
        if (p.ks.S > 1) {
            const int Rx = S - p.ks.bfull;   // the kernel divides by this
            if (p.ks.bfull < 1 || Rx < 1) fail("walk 2: no partial round to split", c, p);
            if (p.ks.bfull % (c.slots / 8)) fail("walk 2: the split does not start at a round of the XCD", c, p);
            if (Rx >= c.slots / 8) fail("walk 2: more than a partial round as quadrants", c, p);
            if (8 * Rx > c.t.ksplit_max) fail("walk 2: tail above ksplit_max", c, p);
            if (p.grid != 8 * S + 24 * Rx) fail("walk 2: grid size", c, p);
        } else if (p.grid != 8 * S) fail("walk 2: grid size", c, p);
        if (sub) fail("walk 2 with sub-tile blocks", c, p);
    }
    // tile (0, 0) belongs to the sub-tile blocks exactly when bit 0x200 is set: they need the tile wholly inside C, K a
    // multiple of 64, a diagonal block to factor, and tile 0 must not be a quadrant tile as well
    if (sub) {
        if (!p.fuse || !c.diag || !(c.t.fuse_diag & 8) || walk != 0 || c.M < GT || c.N < GT || c.K % 64) fail("sub-tile blocks not allowed here", c, p);
        if (p.ks.S > 1 && p.ks.bfull < 1) fail("tile (0, 0) is both sub-tiled and a quadrant tile", c, p);
        if (p.multi_round && (c.t.fuse_diag & 2)) fail("sub-tile blocks in a launch that fuses in block 0", c, p);
    }
    // the fused-block flag: only when tile (0, 0) is computed whole by block 0 or by the sub-tile blocks
    if (p.fuse) {
        if (!c.diag) fail("fused without a diagonal block", c, p);
        if (!sub) {
            if (!p.multi_round || !(c.t.fuse_diag & 2)) fail("fused in block 0 outside a multi-round launch", c, p);
            if (p.ks.S > 1 && p.ks.bfull < 1) fail("fused in block 0, but block 0 is a quadrant", c, p);
            if (walk == 2 && T == 1) fail("fused in block 0 of a one-row band walk", c, p);
        }
    } else if (c.diag && p.multi_round && (c.t.fuse_diag & 2)) fail("a multi-round launch leaves the offered block", c, p);
}

int sweep()
{
    const int lastv[4] = {1, 64, 65, 128}, Ks[3] = {128, 130, 1024}, slots[5] = {8, 16, 24, 40, 512};
    const int orders[2] = {0, 2}, ksplits[2] = {0, 1}, kmax[3] = {0, 8, 100}, fuses[4] = {0, 2, 8, 15};
    for (int T = 1; T <= 40; ++T)
        for (int TN = 1; TN <= T; ++TN) {
            check_walks(T, TN);
            for (int vl : lastv)
                for (int nl : lastv) {
                    Combo c{};
                    c.M = (T - 1) * GT + vl;
                    c.N = (TN - 1) * GT + nl;
                    if (c.N > c.M) continue;  // C is M x N with N <= M
                    for (int K : Ks)
                        for (int sl : slots)
                            for (int o : orders)
                                for (int ksp : ksplits)
                                    for (int km : kmax)
                                        for (int f : fuses)
                                            for (int lanes = 0; lanes < 2; ++lanes)
                                                for (int diag = 0; diag < 2; ++diag) {
                                                    c.K = K; c.slots = sl; c.lanes = lanes; c.diag = diag;
                                                    c.t = SyrkTune{o, (2 << 16) | 4, f, ksp, km};
                                                    check_plan(c);
                                                }
                }
        }
    // the other ends of the plan: empty updates and the upper-triangular panel
    const SyrkTune t{2, (2 << 16) | 4, 15, 1, 100};
    if (syrk_plan(0, 5, 5, 16, t, 0, true, 0).launch || syrk_plan(5, 0, 5, 16, t, 0, true, 0).launch || syrk_plan(5, 5, 0, 16, t, 0, true, 1).launch) {
        ++g_fail;
        printf("VIOLATION an empty update is launched\n");
    }
    for (int n = 1; n <= 5000; n += 61) {
        const SyrkPlan p = syrk_plan(n, n, n, syrk_slots(0), t, 0, true, 1);
        const int T = (n + GT - 1) / GT;
        if (!p.launch || p.order != 0x100 || p.grid != T * (T + 1) / 2 || p.fuse || p.ks.S > 1 || p.stagger) {
            ++g_fail;
            printf("VIOLATION upper-triangular panel n=%d: grid=%d order=0x%x\n", n, p.grid, p.order);
        }
    }
    printf("%ld plans, %d violations\n", g_plans, g_fail);
    return g_fail ? 1 : 0;
}

int classify_stdin()
{
    char line[256];
    while (fgets(line, sizeof line, stdin)) {
        Combo c{};
        int o, ksp, km, f;
        if (sscanf(line, "%d %d %d %d %d %d %d %d %d %d", &c.M, &c.N, &c.K, &c.slots, &o, &ksp, &km, &f, &c.lanes, &c.diag) != 10) {
            fprintf(stderr, "bad line: %s", line);
            return 2;
        }
        c.t = SyrkTune{o, (2 << 16) | 4, f, ksp, km};
        const SyrkPlan p = syrk_plan(c.M, c.N, c.K, c.slots, c.t, c.lanes, c.diag != 0, 0);
        if (!p.launch) {
            printf("empty\n");
            continue;
        }
        const Class k = classify(c, p);
        printf("walk=%d multi=%d tail=%d thin=%d fused=%s shape=%s\n", k.walk, (int)k.multi, (int)k.tail, (int)k.thin, k.fused,
               k.trap ? "trap" : "tri");
    }
    return 0;
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc == 2 && !strcmp(argv[1], "sweep")) return sweep();
    if (argc == 2 && !strcmp(argv[1], "classify")) return classify_stdin();
    fprintf(stderr, "usage: %s sweep | classify < lines\n", argv[0]);
    return 2;
}
