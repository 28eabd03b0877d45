// The arithmetic of the screened ballot check (screen.hip; include/vsp.h "SAVER ballots screened in bulk") that a CPU can
// check: the multiplication of a point by a 128-bit coefficient and the tree that multiplies the Miller values of a range.  Shared by
// the gfx950 kernels (32-bit limbs) and, through g++, by the CPU test build (tests/cpu_build/screen_check.cpp, both limb types).
#pragma once
#include "fp12.h"
#include "curve.h"

namespace vsp {

// z P for z = lo + 2^64 hi, P affine in Montgomery form: 128 doublings from the top bit down and one mixed addition per set bit --
// 128 x 9 + 64 x 10 = 1 800 field products for a random z.  (Wider windows do not pay here: their table entries are not affine, and a
// full addition costs 14 products against the 10 of a mixed one.)  The steps go through dbl_(XYZZ *) and madd_(XYZZ *, const Affine *)
// so that a kernel passes its out-of-line copies (pairing_g1.h pr_dbl / pr_madd); every exceptional case is theirs (curve.h): P at
// infinity or z = 0 gives infinity
template <class F, class Dbl, class Madd>
VSP_HD void screen_mul128(XYZZ<F> &acc, const Affine<F> &P, uint64_t lo, uint64_t hi, Dbl dbl_, Madd madd_) {
    acc = XYZZ<F>::inf();
#if defined(__HIPCC__)
#pragma unroll 1
#endif
    for (int i = 127; i >= 0; i--) {
        dbl_(&acc);
        if (((i < 64 ? lo : hi) >> (i & 63)) & 1) madd_(&acc, &P);
    }
}

// THE PRODUCT TREE.  The Miller values of a range are multiplied level by level: value t of the next level is the product of the
// values [t SCREEN_FAN, min((t + 1) SCREEN_FAN, count)) of this one, so a range of 2^16 values takes four levels of at most 16
// dependent products instead of one chain of 65 535.
static constexpr size_t SCREEN_FAN = 16;
VSP_HD size_t screen_level_count(size_t count) { return (count + SCREEN_FAN - 1) / SCREEN_FAN; }
// value t of the next level; mul_(Fp12 *f, const Fp12 *g) is f = f g
template <class F, class Mul>
VSP_HD Fp12T<F> screen_segment_product(const Fp12T<F> *in, size_t count, size_t t, Mul mul_) {
    const size_t first = t * SCREEN_FAN, last = first + SCREEN_FAN < count ? first + SCREEN_FAN : count;
    Fp12T<F> f = in[first];
#if defined(__HIPCC__)
#pragma unroll 1
#endif
    for (size_t i = first + 1; i < last; i++) { Fp12T<F> g = in[i]; mul_(&f, &g); }
    return f;
}
// A LIST of equal ranges goes through the tree together.  Range r of a level holds `count(r)` values from in[r stride] on: at level 0
// the ranges lie back to back (stride = len, the last range may be shorter); a level of stride s is followed by one of stride
// screen_level_count(s).  Levels follow until the stride is 1: then value r is the product of range r.
struct ScreenLevel {
    size_t ranges, stride, count_full, count_last;                  // count_last: the last range's
    VSP_HD size_t count(size_t r) const { return r + 1 == ranges ? count_last : count_full; }
    VSP_HD ScreenLevel next() const { return ScreenLevel{ranges, screen_level_count(stride), screen_level_count(count_full), screen_level_count(count_last)}; }
};
// the first level over `total` values in ranges of `len` (the last one holds what is left)
VSP_HD ScreenLevel screen_first_level(size_t total, size_t len) {
    const size_t ranges = (total + len - 1) / len;
    return ScreenLevel{ranges, len, len, total - (ranges - 1) * len};
}

}  // namespace vsp
