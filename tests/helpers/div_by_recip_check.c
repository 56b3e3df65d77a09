/* Exhaustive check of the kernels' division shortcut (nus_device.hpp: div_by_recip): q = RN(x z), r = fma(-y, q, x),
 * result = fma(r, z, q) with z = RN(1 / y) against the IEEE quotient x / y, over every mantissa of x (three binades, both
 * signs) for the divisors the kernels use it with: 9 (Horn-Schunck mean), 255 (unorm8), the all-ones mantissa (the
 * exception of Markstein's theorem, which a Horn-Schunck denominator can hit) and a spread of ordinary mantissas.
 * Inside its proven domain (x = +0 or 2^-100 <= |x| <= 2^100, 2^-24 <= y <= 2^24) the sequence is invariant under scaling x
 * or y by a power of two, so mantissas are all that matters there.
 *
 * Part 2 checks the guarded form the Horn-Schunck kernels call (div_exact / div_exact_recip: the sequence inside the domain,
 * the plain division outside) ACROSS the exponent range: every mantissa of x, for y = 9 and for a Horn-Schunck denominator, in
 * the binades that hold subnormal x, the smallest normals, both thresholds and their neighbours and the largest finite values; every binade of x (subnormals
 * included) against divisors from 2^-30 to 2^30 -- the domain's ends 2^-24 and 2^24, the largest value below 2^25, divisors
 * outside it -- so that subnormal quotients, quotients at the thresholds and overflowing quotients all occur; and the special
 * values (+-0, +-inf, NaN).  It also counts how often the UNGUARDED sequence misses the quotient of a subnormal or tiny x: that
 * must happen, or this program could not see the defect the guard is there for.
 * Prints "ok <checked> guarded <checked in part 2> unguarded_bad <count>" or "bad <count> ..."; test infrastructure only. */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

static float asf(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
static uint32_t asu(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static float div_by_recip(float x, float y, float z)
{
    const float q = x * z;
    const float r = fmaf(-y, q, x);
    return fmaf(r, z, q);
}
static float div_exact_recip(float y) { return (y >= 0x1p-24f && y <= 0x1p+24f) ? 1.0f / y : -1.0f; }
static float div_exact(float x, float y, float z)
{
    const float a = fabsf(x);
    const int proven = ((a >= 0x1p-100f && a <= 0x1p+100f) || asu(x) == 0u) && z > 0.0f;
    if (proven) return div_by_recip(x, y, z);
    return x / y;
}
/* same bits, or both NaN (the payload of a NaN is not part of the contract) */
static int same(float a, float b) { return asu(a) == asu(b) || (a != a && b != b); }

int main(void)
{
    uint32_t ys[40];
    int ny = 0;
    ys[ny++] = asu(9.0f);
    ys[ny++] = asu(255.0f);
    ys[ny++] = 0x3FFFFFFFu; /* mantissa all ones */
    ys[ny++] = 0x3FFFFFFEu;
    ys[ny++] = 0x3F800001u;
    uint32_t s = 12345u;
    while (ny < 40) { s = s * 1664525u + 1013904223u; ys[ny++] = 0x3F800000u | (s >> 9); }
    unsigned long long checked = 0, bad = 0;
    for (int k = 0; k < ny; ++k) {
        const float y = asf(ys[k]), z = 1.0f / y;
        const uint32_t step = k < 3 ? 1u : 7u; /* the three named divisors exhaustively, the others every 7th mantissa */
        for (uint32_t e = 0; e < 3; ++e)
            for (uint32_t m = 0; m < (1u << 23); m += step) {
                const float x = asf(((126u + e) << 23) | m);
                if (asu(div_by_recip(x, y, z)) != asu(x / y)) ++bad;
                if (asu(div_by_recip(-x, y, z)) != asu(-x / y)) ++bad;
                checked += 2;
            }
    }

    /* ---- part 2: the guarded form across the exponent range ---- */
    unsigned long long guarded = 0, unguarded_bad = 0;
    {
        /* y = 9 and a Horn-Schunck denominator with a full mantissa (lambda + 0.25), every mantissa of x: biased exponent
         * 0 = subnormal x, 1 and 3 = quotient subnormal or just normal, 26 .. 28 around the lower threshold 2^-100 (27), 227 and
         * 228 around the upper one 2^100 (227), 254 = the largest finite binade.  (x / 9 survives the unguarded sequence even
         * for subnormal x -- 9 q is a multiple of 2^-149 whenever q is --; a divisor with low mantissa bits does not.) */
        static const uint32_t exps[] = {0, 1, 3, 26, 27, 28, 227, 228, 254};
        const float yy[2] = {9.0f, 4e-4f + 0.25f};
        for (int k = 0; k < 2; ++k) {
            const float y = yy[k], z = div_exact_recip(y);
            for (unsigned i = 0; i < sizeof exps / sizeof exps[0]; ++i)
                for (uint32_t m = 0; m < (1u << 23); ++m) {
                    const float x = asf((exps[i] << 23) | m);
                    if (!same(div_exact(x, y, z), x / y)) ++bad;
                    if (!same(div_exact(-x, y, z), -x / y)) ++bad;
                    guarded += 2;
                    if (exps[i] < 26 && (exps[i] | m) != 0 && asu(div_by_recip(x, y, 1.0f / y)) != asu(x / y)) ++unguarded_bad;
                }
        }
    }
    {
        /* every binade of x, 4099 mantissas each (first, last and a stride), against divisors of every size */
        uint32_t yd[160];
        int nd = 0;
        static const uint32_t mant[] = {0u, 1u, 0x7FFFFFu, 0x7FFFFEu, 0x100000u, 0x2AAAABu, 0x555555u, 0x6DB6DBu};
        for (int e = -30; e <= 30; e += 3)
            for (unsigned j = 0; j < 4; ++j) yd[nd++] = ((uint32_t)(127 + e) << 23) | mant[(j + (unsigned)(e + 30)) % 8u];
        yd[nd++] = asu(0x1p-24f);                /* the domain's ends, the values next to them on either side */
        yd[nd++] = asu(0x1p-24f) - 1u;
        yd[nd++] = asu(0x1p-24f) + 1u;
        yd[nd++] = asu(0x1p+24f);
        yd[nd++] = asu(0x1p+24f) - 1u;
        yd[nd++] = asu(0x1p+24f) + 1u;
        yd[nd++] = asu(0x1p+25f) - 1u;
        yd[nd++] = asu(4e-4f);                   /* Horn-Schunck denominators: lambda .. lambda + 0.5 */
        yd[nd++] = asu(4e-4f + 0.25f);
        yd[nd++] = asu(1e-6f);
        yd[nd++] = asu(1.0f);
        yd[nd++] = asu(0.0f);                    /* a divisor no reciprocal exists for: the plain path's inf / NaN */
        yd[nd++] = asu(-3.0f);
        for (int k = 0; k < nd; ++k) {
            const float y = asf(yd[k]), z = div_exact_recip(y);
            for (uint32_t e = 0; e <= 254; ++e)
                for (uint32_t m = 0; m < (1u << 23); m += 2047u) {
                    for (int edge = 0; edge < 2; ++edge) { /* m, and the same distance from the binade's top */
                        const float x = asf((e << 23) | (edge ? 0x7FFFFFu - m : m));
                        if (!same(div_exact(x, y, z), x / y)) ++bad;
                        if (!same(div_exact(-x, y, z), -x / y)) ++bad;
                        guarded += 2;
                    }
                }
        }
        /* the thresholds themselves, their neighbours, and the special values */
        static const uint32_t xs[] = {0x00000000u, 0x80000000u, 0x00000001u, 0x007FFFFFu, 0x00800000u, 0x7F7FFFFFu, 0x7F800000u,
                                      0xFF800000u, 0x7FC00000u, 0x0D800000u /* 2^-100 */, 0x0D7FFFFFu, 0x0D800001u,
                                      0x71800000u /* 2^100 */, 0x717FFFFFu, 0x71800001u};
        for (int k = 0; k < nd; ++k)
            for (unsigned i = 0; i < sizeof xs / sizeof xs[0]; ++i) {
                const float y = asf(yd[k]), x = asf(xs[i]);
                if (!same(div_exact(x, y, div_exact_recip(y)), x / y)) ++bad;
                ++guarded;
            }
    }
    if (asf(0x0D800000u) != 0x1p-100f || asf(0x71800000u) != 0x1p+100f) ++bad; /* the table above names the thresholds */
    if (unguarded_bad == 0) { printf("bad: the unguarded sequence matched every tiny quotient -- this check sees nothing\n"); return 1; }
    if (bad) printf("bad %llu of %llu\n", bad, checked + guarded);
    else printf("ok %llu guarded %llu unguarded_bad %llu\n", checked, guarded, unguarded_bad);
    return bad != 0;
}
