// CPU test build of the device square root (fp_sqrt.h compiled by g++ with the 32-bit-limb type the decoding kernel uses, and
// with the host's 64-bit-limb type).  Test infrastructure only.  All arguments canonical little-endian u64 limbs.
#include <string.h>
#include "../../vote_saver_protocol_amd/csrc/fp_sqrt.h"
using namespace vsp;

template <class T> static T load(const uint64_t *p) { T t; memcpy(&t, p, sizeof(T)); return t; }
template <class T> static void store(uint64_t *p, const T &t) { memcpy(p, &t, sizeof(T)); }

// out = a^((p+1)/4); returns 1 when that is a square root of a
template <class F> static int sqrt_of(const uint64_t *a, uint64_t *out) {
    F y;
    const bool ok = fp_sqrt(to_mont(load<F>(a)), y);
    store(out, from_mont(y));
    return ok ? 1 : 0;
}
// out = the y of the compressed point (x, larger); returns 1 when x is the abscissa of a curve point
template <class F> static int y_of(const uint64_t *x, int larger, uint64_t *out) {
    F y;
    const bool ok = g1_y_from_x(to_mont(load<F>(x)), larger != 0, y);
    store(out, from_mont(y));
    return ok ? 1 : 0;
}
extern "C" {
int chk_fp_sqrt(const uint64_t *a, uint64_t *out) { return sqrt_of<Fp>(a, out); }
int chk_hfp_sqrt(const uint64_t *a, uint64_t *out) { return sqrt_of<HFp>(a, out); }
int chk_g1_y(const uint64_t *x, int larger, uint64_t *out) { return y_of<Fp>(x, larger, out); }
int chk_hg1_y(const uint64_t *x, int larger, uint64_t *out) { return y_of<HFp>(x, larger, out); }
int chk_fp_above_half(const uint64_t *a) { return fp_canon_above_half(load<Fp>(a)) ? 1 : 0; }
}
