// The bisector split of a two-centre cube (kmeans.hip, split_drain) from a table per centre pair,
// written once for the Lloyd kernel and for the host check (tools/km_lattice_check.cpp).
//
// For owner k and contender j the split needs, at the cube's 64 positions u = (i, j', b), the sign
// of the fixed-point form
//     F(u) = F0q + gx i + gy j' + gz b,      (gx, gy, gz) = rint((c_k - c_j) 2^(kFrac + 1)),
// against the band: F > kBand labels k, F < -kBand labels j, the rest is left to the caller.  The
// steps depend on the centre pair alone; only F0q is the cube's own.  So the 16 values
//     v(q) = gy j' + gz b,  q = 4 j' + b,
// are sorted once per pair, and in slice i
//     "surely k" = {v > kBand - F0q - gx i}   is a suffix of the sorted order,
//     "surely j" = {v < -kBand - F0q - gx i}  a prefix:
// a rank among 16 sorted values and one 16-bit mask per side and slice, instead of 64 steps per
// cube.  Everything is int32 in 2^-kFrac units and nothing is rounded, so the masks are those of
// the position-by-position walk bit for bit.
//
// One table serves both orders of a pair.  It is built for (lo, hi), lo < hi, from c_lo - c_hi.
// For owner hi and contender lo the walk's steps are rint((c_hi - c_lo) 2^(kFrac + 1)).  IEEE
// subtraction gives c_hi - c_lo = -(c_lo - c_hi) exactly (the same real number with the sign
// flipped, rounded to nearest either way), the scaling by a power of two is exact at these
// magnitudes, and rintf (round half to even) is an odd function: the reversed pair's steps are
// exactly -gx, -gy, -gz, its values -v.  With A = kBand -+ F0q - gx i (the table's gx; minus for
// owner lo, plus for owner hi) both orders read
//     S = {v > A}             the colours that are surely c_lo's,
//     P = {v <= A - 2 kBand - 1} = {v < A - 2 kBand}   surely c_hi's,
// and only which of the two is the owner's side differs.
//
// |g| <= 255 x 2^11 = 522 240, |v| <= 6 |g|, |F0q| < 2^29: no sum here leaves int32.
#ifndef LLFE_KMEANS_LATTICE_H
#define LLFE_KMEANS_LATTICE_H
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define LLFE_KML_HD __host__ __device__ __forceinline__
#else
#define LLFE_KML_HD inline
#endif

namespace llfe_kml {

constexpr int kFrac = 10;               // fractional bits of F (kmeans.hip: kBisFrac)
constexpr int kBand = 1 << (kFrac - 1);  // 0.5 (kBisBand)

// The table of one unordered centre pair, 144 B: the stride keeps the ten tables of a workgroup on
// distinct LDS banks for the 16-byte reads.
struct alignas(16) PairTable {
    int32_t c[4];     // v[3], v[7], v[11], v[15]: the first of the two search levels, one 16-byte read
    int32_t gxy[2];   // gx, gy
    int32_t vb[18];   // INT32_MIN twice, then the values v(q), ascending (equal values in the order of q): v[r] = vb[r + 2]
    int32_t gz;
    uint16_t mm[18];  // mm[r + 1] = m[r], r <= 16: the positions q of sorted rank >= r (m[0] = 0xFFFF, m[16] = 0); mm[0] = 0xFFFF stands for
                      // m[-1]: a slice of rank 0 reads it beside m[0] and never uses it (no value lies below v[0])
    uint32_t pad[2];
};
static_assert(sizeof(PairTable) == 144, "PairTable layout");

// index of the pair (lo, hi), lo < hi < 5: (0,1) (0,2) (0,3) (0,4) (1,2) ... (3,4)
LLFE_KML_HD int pair_index(int lo, int hi) { return ((lo * (9 - lo)) >> 1) + hi - lo - 1; }
LLFE_KML_HD int pair_lo(int p) { return (p >= 4) + (p >= 7) + (p >= 9); }
LLFE_KML_HD int pair_hi(int p) {
    const int lo = pair_lo(p);
    return p - ((lo * (9 - lo)) >> 1) + lo + 1;
}

// a step of F for one coordinate of the pair, by split_drain's own expression
LLFE_KML_HD int lattice_step(float c_lo, float c_hi) {
    return (int)__builtin_rintf((c_lo - c_hi) * (2.f * (float)(1 << kFrac)));
}
LLFE_KML_HD int lattice_value(int q, int gy, int gz) { return gy * (q >> 2) + gz * (q & 3); }
// the sorted rank of position q: the positions with a smaller value, or an equal one and a smaller q
LLFE_KML_HD int lattice_rank(int q, int gy, int gz) {
    const int v = lattice_value(q, gy, gz);
    int r = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int o = 0; o < 16; o++) {
        const int w = lattice_value(o, gy, gz);
        r += (w < v) | ((w == v) & (o < q));
    }
    return r;
}

// Position q's share of the table of a pair with steps (gx, gy, gz): its value at its sorted rank (and in the
// coarse level when the rank ends a quarter), its own bit where the rank's mask will be, and, from position 0,
// what does not depend on a position.  The kernel gives each of 16 lanes one position; the masks are then the
// suffix OR of the bits, mm[r + 1] |= mm[r + 2] ... (there along the 16-lane row, in lattice_build by a loop).
LLFE_KML_HD void lattice_place(PairTable &t, int q, int gx, int gy, int gz) {
    const int v = lattice_value(q, gy, gz), r = lattice_rank(q, gy, gz);
    t.vb[r + 2] = v;
    if ((r & 3) == 3) t.c[r >> 2] = v;
    t.mm[r + 1] = (uint16_t)(1u << q);
    if (q == 0) {
        t.gxy[0] = gx, t.gxy[1] = gy, t.gz = gz;
        t.vb[0] = t.vb[1] = INT32_MIN;
        t.mm[0] = 0xFFFF, t.mm[17] = 0;
    }
}

// The whole table by one thread (the host check's build).
LLFE_KML_HD void lattice_build(const float c_lo[3], const float c_hi[3], PairTable &t) {
    const int gx = lattice_step(c_lo[0], c_hi[0]), gy = lattice_step(c_lo[1], c_hi[1]), gz = lattice_step(c_lo[2], c_hi[2]);
    for (int q = 0; q < 16; q++) lattice_place(t, q, gx, gy, gz);
    for (int r = 14; r >= 0; r--) t.mm[r + 1] = (uint16_t)(t.mm[r + 1] | t.mm[r + 2]);
    t.pad[0] = t.pad[1] = 0u;
}

// n + (v <= a).  On the device a compare and an add with carry, two instructions: the compiler's own form of
// the counts below (select 0 / 1, pack pairs, packed 16-bit adds) came to three per compare.
LLFE_KML_HD int count_le(int n, int v, int a) {
#if defined(__HIP_DEVICE_COMPILE__)
    asm("v_cmp_le_i32 vcc, %1, %2\n\tv_addc_co_u32 %0, vcc, 0, %0, vcc" : "+v"(n) : "v"(v), "v"(a) : "vcc");
    return n;
#else
    return n + (v <= a);
#endif
}

// four consecutive table words from a 16-byte aligned address, one read
struct __attribute__((aligned(16), may_alias)) Quad {
    int32_t x, y, z, w;
};
static_assert(offsetof(PairTable, c) % 16 == 0 && offsetof(PairTable, vb) % 16 == 8, "the 16-byte reads of PairTable");

// r[s] = the number of table values <= a[s], for the four slices at once: the coarse level from one
// 16-byte read shared by the slices, then the four values of the slice's own quarter.
LLFE_KML_HD void lattice_ranks(const PairTable &t, const int a[4], int r[4]) {
    const Quad c = *reinterpret_cast<const Quad *>(&t.c[0]);
    int h[4];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int s = 0; s < 4; s++) {
        const int n = count_le(count_le(count_le(count_le(0, c.x, a[s]), c.y, a[s]), c.z, a[s]), c.w, a[s]);
        h[s] = n < 3 ? n : 3;  // (all of the last quarter <= a: 12 + 4)
    }
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int s = 0; s < 4; s++) {
        const Quad b = reinterpret_cast<const Quad *>(&t.vb[2])[h[s]];
        r[s] = count_le(count_le(count_le(count_le(4 * h[s], b.x, a[s]), b.y, a[s]), b.z, a[s]), b.w, a[s]);
    }
}

// The split of one cube: lo_side = the positions (bit = 16 i + q) that are surely c_lo's, x | y << 32,
// hi_side = those that are surely c_hi's.  owner_hi: the cube's owner is the pair's larger index (F0q is
// always the owner's form, d_contender - d_owner at the cube's origin).
struct Sides {
    uint32_t lo_x, lo_y, hi_x, hi_y;
};
LLFE_KML_HD Sides lattice_sides(int f0q, const PairTable &t, bool owner_hi) {
    const int gx = t.gxy[0];
    const int a0 = kBand + (owner_hi ? f0q : -f0q);
    int a[4], b[4], ra[4];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int s = 0; s < 4; s++) {
        a[s] = a0 - gx * s;
        b[s] = a[s] - (2 * kBand + 1);
    }
    lattice_ranks(t, a, ra);
    // The other side ends at rb = the number of values <= b, and ra - rb values lie inside the band (b < v <= a):
    // mostly none, sometimes one.  Beside the mask m[ra] the lane reads m[ra - 1] and the two largest values
    // <= a, v[ra - 1] and v[ra - 2] (INT32_MIN below v[0]): they settle rb = ra and rb = ra - 1 without another
    // dependent read.  Only a slice with two or more values inside the band (equal or nearly equal values:
    // a pair whose centres differ along one axis only) walks down from there.
    uint32_t ma[4], mb[4];
    int rb[4], pv[4];
    bool deep[4];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int s = 0; s < 4; s++) {
        const int p2 = t.vb[ra[s]], p1 = t.vb[ra[s] + 1];
        const uint32_t m1 = t.mm[ra[s]], m0 = t.mm[ra[s] + 1];
        ma[s] = m0;
        mb[s] = p1 > b[s] ? m1 : m0;
        rb[s] = ra[s] - 1;  // (where the walk below starts: v[ra - 1] is inside the band there)
        pv[s] = p2;
        deep[s] = p2 > b[s];
    }
    if (deep[0] | deep[1] | deep[2] | deep[3]) {
        do {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
            for (int s = 0; s < 4; s++) {
                if (pv[s] > b[s]) {
                    rb[s]--;
                    pv[s] = t.vb[rb[s] + 1];
                }
            }
        } while ((pv[0] > b[0]) | (pv[1] > b[1]) | (pv[2] > b[2]) | (pv[3] > b[3]));
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (int s = 0; s < 4; s++)
            if (deep[s]) mb[s] = t.mm[rb[s] + 1];
    }
    Sides o;
    o.lo_x = ma[0] | (ma[1] << 16);
    o.lo_y = ma[2] | (ma[3] << 16);
    o.hi_x = ~(mb[0] | (mb[1] << 16));
    o.hi_y = ~(mb[2] | (mb[3] << 16));
    return o;
}

// What the 64-step walk returns for owner k and contender j: x | y << 32 = F > kBand, z | w << 32 =
// F < -kBand.
struct Signs {
    uint32_t x, y, z, w;
};
LLFE_KML_HD Signs lattice_signs(int f0q, const PairTable &t, bool owner_hi) {
    const Sides s = lattice_sides(f0q, t, owner_hi);
    return owner_hi ? Signs{s.hi_x, s.hi_y, s.lo_x, s.lo_y} : Signs{s.lo_x, s.lo_y, s.hi_x, s.hi_y};
}

}  // namespace llfe_kml
#endif
