// Host check of csrc/kmeans_lattice.h: the pair-table lookup of the two-centre cube split against a
// plain restatement of the 64-step walk it replaces (kmeans.hip, bisector_signs), bit for bit.
// Built with AddressSanitizer and UndefinedBehaviorSanitizer by tests/test_kmeans_lattice_host.py.
// Prints one line per family "<name> <lookups> <mismatches>" and "ok" when nothing differed.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>

#include "kmeans_lattice.h"

namespace {
using namespace llfe_kml;

// the walk: from position 63 down, one add per position, the sign bits of band - F and of F + band
Signs walk(int f0q, int gx, int gy, int gz) {
    int p = kBand - (f0q + 3 * (gx + gy + gz));
    int n = 2 * kBand - p;
    const int s1 = gz, s2 = gy - 3 * gz, s3 = gx - 3 * (gy + gz);
    uint32_t w[4] = {0u, 0u, 0u, 0u};
    for (int bit = 63; bit >= 0; bit--) {
        const int h = bit >> 5;
        w[h] = (w[h] << 1) | (uint32_t)(p < 0);
        w[2 + h] = (w[2 + h] << 1) | (uint32_t)(n < 0);
        if (bit > 0) {
            const int s = (bit & 15) == 0 ? s3 : ((bit & 3) == 0 ? s2 : s1);
            p += s;
            n -= s;
        }
    }
    return Signs{w[0], w[1], w[2], w[3]};
}

// centres of a pair whose steps are exactly (gx, gy, gz): multiples of 2^-11 in [0, 255]
void centres_of(const int g[3], float lo[3], float hi[3]) {
    for (int d = 0; d < 3; d++) {
        lo[d] = g[d] >= 0 ? (float)g[d] / 2048.f : 0.f;
        hi[d] = g[d] >= 0 ? 0.f : (float)(-g[d]) / 2048.f;
    }
}

struct Family {
    const char *name;
    long long n = 0, bad = 0;
};

// both orders of the pair at one F0q: owner lo walks the table's steps, owner hi the steps of
// c_hi - c_lo formed by the kernel's expression on the swapped centres
void check(Family &f, const float lo[3], const float hi[3], const PairTable &t, int f0q) {
    for (int rev = 0; rev < 2; rev++) {
        const float *ck = rev ? hi : lo, *cj = rev ? lo : hi;
        const int gx = lattice_step(ck[0], cj[0]), gy = lattice_step(ck[1], cj[1]), gz = lattice_step(ck[2], cj[2]);
        const Signs a = walk(f0q, gx, gy, gz), b = lattice_signs(f0q, t, rev != 0);
        f.n++;
        if (a.x != b.x || a.y != b.y || a.z != b.z || a.w != b.w) {
            if (f.bad++ < 5)
                std::printf("MISMATCH %s g %d %d %d f0q %d rev %d walk %08x %08x %08x %08x table %08x %08x %08x %08x\n", f.name,
                            gx, gy, gz, f0q, rev, a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w);
        }
    }
}

// every F0q that puts F within +-2 units of +-band at some position of the cube, for either owner
void check_edges(Family &f, const int g[3]) {
    float lo[3], hi[3];
    centres_of(g, lo, hi);
    PairTable t;
    lattice_build(lo, hi, t);
    for (int u = 0; u < 64; u++) {
        const int L = g[0] * (u >> 4) + g[1] * ((u >> 2) & 3) + g[2] * (u & 3);
        for (int side = -1; side <= 1; side += 2)
            for (int sg = -1; sg <= 1; sg += 2)
                for (int d = -2; d <= 2; d++) check(f, lo, hi, t, sg * (side * kBand + d) - sg * L);
    }
}

void check_random_f(Family &f, const int g[3], std::mt19937_64 &rng, int reps) {
    float lo[3], hi[3];
    centres_of(g, lo, hi);
    PairTable t;
    lattice_build(lo, hi, t);
    std::uniform_int_distribution<int> wide(-(1 << 29) + 1, (1 << 29) - 1), near(-8 * 522240, 8 * 522240);
    for (int r = 0; r < reps; r++) {
        check(f, lo, hi, t, wide(rng));
        check(f, lo, hi, t, near(rng));
    }
}
}  // namespace

int main() {
    std::mt19937_64 rng(20240611u);
    Family fams[8];
    int nf = 0;

    {  // exhaustive small steps
        Family &f = fams[nf++];
        f.name = "small";
        for (int gx = -3; gx <= 3; gx++)
            for (int gy = -3; gy <= 3; gy++)
                for (int gz = -3; gz <= 3; gz++) {
                    const int g[3] = {gx, gy, gz};
                    check_edges(f, g);
                }
    }
    {  // zero steps in y and z (16 equal values), all steps equal, multiples of 512
        Family &f = fams[nf++];
        f.name = "ties";
        std::uniform_int_distribution<int> full(-522240, 522240), k512(-1020, 1020);
        for (int r = 0; r < 400; r++) {
            const int a = full(rng), m = k512(rng) * 512, m2 = k512(rng) * 512;
            const int sets[6][3] = {{a, 0, 0}, {0, 0, 0}, {a, a, a}, {0, a, a}, {m, m2, m}, {m, m, -m}};
            for (const auto &g : sets) {
                check_edges(f, g);
                check_random_f(f, g, rng, 4);
            }
        }
    }
    {  // tiny steps at random F0q and at the band's edges
        Family &f = fams[nf++];
        f.name = "tiny";
        std::uniform_int_distribution<int> tiny(-40, 40);
        for (int r = 0; r < 2000; r++) {
            const int g[3] = {tiny(rng), tiny(rng), tiny(rng)};
            check_edges(f, g);
        }
    }
    {  // full range
        Family &f = fams[nf++];
        f.name = "random";
        std::uniform_int_distribution<int> full(-522240, 522240);
        for (int r = 0; r < 120000; r++) {
            const int g[3] = {full(rng), full(rng), full(rng)};
            check_random_f(f, g, rng, 1);
            if (r % 64 == 0) check_edges(f, g);
        }
    }
    {  // arbitrary float32 centres: the reversed pair's steps are the table's, negated
        Family &f = fams[nf++];
        f.name = "float_centres";
        std::uniform_real_distribution<float> col(0.f, 255.f);
        std::uniform_int_distribution<int> near(-8 * 522240, 8 * 522240);
        for (int r = 0; r < 100000; r++) {
            float lo[3], hi[3];
            for (int d = 0; d < 3; d++) lo[d] = col(rng), hi[d] = col(rng);
            PairTable t;
            lattice_build(lo, hi, t);
            const int g[3] = {t.gxy[0], t.gxy[1], t.gz};
            for (int d = 0; d < 3; d++) {
                f.n++;
                if (lattice_step(hi[d], lo[d]) != -g[d]) f.bad++;
            }
            check(f, lo, hi, t, near(rng));
        }
    }
    {  // pair numbering
        Family &f = fams[nf++];
        f.name = "pairs";
        int p = 0;
        for (int lo = 0; lo < 5; lo++)
            for (int hi = lo + 1; hi < 5; hi++, p++) {
                f.n++;
                if (pair_index(lo, hi) != p || pair_lo(p) != lo || pair_hi(p) != hi) f.bad++;
            }
    }
    long long bad = 0;
    for (int i = 0; i < nf; i++) {
        std::printf("%s %lld %lld\n", fams[i].name, fams[i].n, fams[i].bad);
        bad += fams[i].bad;
    }
    if (bad) return 1;
    std::printf("ok\n");
    return 0;
}
