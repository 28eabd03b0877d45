// CPU test build of the device square root in Fp2 (fp2_sqrt.h compiled by g++ with the 32-bit-limb type the G2 decoding kernel
// uses, and with the host's 64-bit-limb type).  Test infrastructure only.  All arguments canonical little-endian u64 limbs, an Fp2
// value as c0 | c1 (12 words).
#include <string.h>
#include "../../vote_saver_protocol_amd/csrc/fp2_sqrt.h"
using namespace vsp;

template <class T> static T load(const uint64_t *p) { T t; memcpy(&t, p, sizeof(T)); return t; }
template <class T> static void store(uint64_t *p, const T &t) { memcpy(p, &t, sizeof(T)); }

// out = the root fp2_sqrt picks; returns its verdict
template <class F2> static int sqrt_of(const uint64_t *a, uint64_t *out) {
    F2 y;
    const bool ok = fp2_sqrt(to_mont(load<F2>(a)), y);
    store(out, from_mont(y));
    return ok ? 1 : 0;
}
// out = the y of the compressed point (x, larger); returns 1 when x is the abscissa of a curve point
template <class F2> static int y_of(const uint64_t *x, int larger, uint64_t *out) {
    F2 y;
    const bool ok = g2_y_from_x(to_mont(load<F2>(x)), larger != 0, y);
    store(out, from_mont(y));
    return ok ? 1 : 0;
}
extern "C" {
int chk_fp2_sqrt(const uint64_t *a, uint64_t *out) { return sqrt_of<Fp2>(a, out); }
int chk_hfp2_sqrt(const uint64_t *a, uint64_t *out) { return sqrt_of<HFp2>(a, out); }
int chk_g2_y(const uint64_t *x, int larger, uint64_t *out) { return y_of<Fp2>(x, larger, out); }
int chk_hg2_y(const uint64_t *x, int larger, uint64_t *out) { return y_of<HFp2>(x, larger, out); }
int chk_fp2_larger(const uint64_t *a) { return fp2_canon_larger(load<Fp2>(a)) ? 1 : 0; }
int chk_hfp2_larger(const uint64_t *a) { return fp2_canon_larger(load<HFp2>(a)) ? 1 : 0; }
}
