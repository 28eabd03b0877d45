"""TEST INFRASTRUCTURE -- regenerates tests/golden/*.json from the pure-Python big-int oracle.

The reference tree holds no vectors for this path, so these fixtures are the
build's own: produced by oracle/bls12_381.py (independent of both the C restatement and the HIP code),
committed, and checked by the CPU tests (C oracle vs fixture) and the GPU tests (HIP path vs fixture).
Run:  python oracle/gen_golden.py
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bls12_381 as o  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden")


def hx(v):
    return "%x" % v


def pt1(p):
    return None if p is None else [hx(p[0]), hx(p[1])]


def pt2(p):
    return None if p is None else [[hx(p[0][0]), hx(p[0][1])], [hx(p[1][0]), hx(p[1][1])]]


def main():
    os.makedirs(OUT, exist_ok=True)
    gen = o.splitmix64(20260101)

    def rfr():
        return o.rand_fr(gen)

    def rfp():
        return (rfr() * rfr() + rfr()) % o.P

    # ---- field vectors
    fp_edge = [0, 1, 2, o.P - 1, o.P - 2, (o.P - 1) // 2, (1 << 380)]
    fr_edge = [0, 1, 2, o.R - 1, o.R - 2, (o.R - 1) // 2, (1 << 254)]
    fp_cases = [(a, b) for a in fp_edge for b in fp_edge[:4]] + [(rfp(), rfp()) for _ in range(24)]
    fr_cases = [(a, b) for a in fr_edge for b in fr_edge[:4]] + [(rfr(), rfr()) for _ in range(24)]
    field = {
        "fp": [{"a": hx(a), "b": hx(b), "mul": hx(a * b % o.P), "add": hx((a + b) % o.P), "sub": hx((a - b) % o.P),
                "inv_a": hx(pow(a, o.P - 2, o.P))} for a, b in fp_cases],
        "fr": [{"a": hx(a), "b": hx(b), "mul": hx(a * b % o.R), "add": hx((a + b) % o.R), "sub": hx((a - b) % o.R),
                "inv_a": hx(pow(a, o.R - 2, o.R))} for a, b in fr_cases],
    }
    fp2_cases = [((rfp(), rfp()), (rfp(), rfp())) for _ in range(12)] + [((0, 1), (0, 1)), ((o.P - 1, 0), (5, o.P - 1))]
    field["fp2"] = [{"a": [hx(a[0]), hx(a[1])], "b": [hx(b[0]), hx(b[1])],
                     "mul": [hx(x) for x in o.Fp2Ops.mul(a, b)], "sqr_a": [hx(x) for x in o.Fp2Ops.sqr(a)],
                     "inv_a": [hx(x) for x in o.Fp2Ops.inv(a)]} for a, b in fp2_cases]
    json.dump(field, open(os.path.join(OUT, "field.json"), "w"), indent=0)

    # ---- curve vectors
    curve = {}
    for name, cur, enc in (("g1", o.G1, pt1), ("g2", o.G2, pt2)):
        P1 = cur.mul(cur.gen, rfr()); P2 = cur.mul(cur.gen, rfr())
        k = rfr()
        curve[name] = {
            "gen": enc(cur.gen), "P1": enc(P1), "P2": enc(P2),
            "P1_plus_P2": enc(cur.add(P1, P2)), "dbl_P1": enc(cur.add(P1, P1)),
            "P1_minus_P1": enc(cur.add(P1, cur.neg(P1))), "k": hx(k), "k_P1": enc(cur.mul(P1, k)),
            "r_minus_1_gen": enc(cur.mul(cur.gen, o.R - 1)),
        }
    json.dump(curve, open(os.path.join(OUT, "curve.json"), "w"), indent=0)

    # ---- MSM vectors: bases k_i*G, scalars with edge cases (0, 1, r-1, duplicates, inverse points, infinity)
    msm = []
    for name, cur, enc in (("g1", o.G1, pt1), ("g2", o.G2, pt2)):
        for n in ((1, 2, 3, 17, 64) if name == "g1" else (1, 3, 17)):
            ks = [rfr() for _ in range(n)]
            ss = [rfr() for _ in range(n)]
            pts = [cur.mul(cur.gen, k) for k in ks]
            if n >= 17:
                ss[0] = 0; ss[1] = 1; ss[2] = o.R - 1; ss[3] = 1
                pts[5] = pts[4]                       # duplicate base
                pts[7] = cur.neg(pts[6]); ss[7] = ss[6]   # inverse pair with equal scalars: cancels
                pts[8] = None                         # infinity base
                ss[9] = ss[10]                        # equal scalars
            res = cur.msm_naive(pts, ss)
            msm.append({"group": name, "n": n, "bases": [enc(p) for p in pts], "scalars": [hx(s) for s in ss], "result": enc(res)})
    json.dump(msm, open(os.path.join(OUT, "msm.json"), "w"), indent=0)

    # ---- NTT vectors (n in 2, 4, 8 against the O(n^2) DFT as well; 1024 by the radix-2 routine)
    nttv = []
    for n in (1, 2, 4, 8, 1024):
        a = [rfr() for _ in range(n)]
        if n >= 8:
            a[0] = 0; a[1] = o.R - 1
        lg = n.bit_length() - 1
        fwd = o.ntt(a)
        if n <= 8:
            assert fwd == o.dft_naive(a, o.fr_root_of_unity(lg))
        nttv.append({"n": n, "input": [hx(x) for x in a], "fft": [hx(x) for x in fwd],
                     "inverse_fft": [hx(x) for x in o.ntt(a, inverse=True)],
                     "coset_fft_g7": [hx(x) for x in o.ntt(a, coset=7)],
                     "inverse_coset_fft_g7": [hx(x) for x in o.ntt(a, inverse=True, coset=7)]})
    json.dump(nttv, open(os.path.join(OUT, "ntt.json"), "w"), indent=0)
    cofactor_points()
    print("golden fixtures written to", os.path.normpath(OUT))


# ---- curve points OUTSIDE the order-r subgroups, of every small cofactor order (cofactor_points.json)
# z = -BLS_X.  #E(Fp) = h1 r with h1 = (z - 1)^2 / 3 = 3 . 11^2 . 10177^2 . 859267^2 . 52437899^2;
# #E'(Fp2) = h2 r with h2 = (z^8 - 4 z^7 + 5 z^6 - 4 z^4 + 6 z^3 - 4 z^2 - 4 z + 13) / 9 = 13^2 . 23^2 . 2713 . 11953 . 262069 . c448
# (c448: the remaining 448-bit factor, taken as it is).  Both are the published cofactors of BLS12-381; the products are asserted below.
G1_COFACTOR_PRIMES = (3, 11, 10177, 859267, 52437899)
G2_COFACTOR_PRIMES = (13, 23, 2713, 11953, 262069)
# Points of order q^2: none exist.  For every squared prime of either cofactor (G1: 11, 10177, 859267, 52437899; G2: 13, 23)
# (#E / q^2) Q had order <= q for each of the first 12 curve points Q (point_of_order_q2): the q-part of the group is (Z/q)^2, not
# cyclic, so the fixture holds no q^2 record.
SUBGROUP_SCALAR = 0x5EED5EED5EED5EED5EED                  # S = SUBGROUP_SCALAR . generator, the fixed subgroup point of the S + T_q records


def curve_points(cur):
    """the curve points with x = 1, 2, 3, ... (G2: x = (k, 1)), both square roots' first, in that order"""
    k = 0
    while True:
        k += 1
        if cur is o.G1:
            x = k
            y = o.fp_sqrt((x * x * x + o.B1) % o.P)
        else:
            x = (k, 1)
            y = o.fp2_sqrt(o.Fp2Ops.add(o.Fp2Ops.mul(o.Fp2Ops.sqr(x), x), o.B2))
        if y is not None:
            assert cur.is_on_curve((x, y))
            yield (x, y)


def q_part(order, q):
    e = 0
    while order % q ** (e + 1) == 0:
        e += 1
    return q ** e


def point_of_order(cur, order, q, label):
    """a point of order q (q prime, or the unfactored c448) from the first found curve point Q with a q-component: (#E / q^e) Q for the
    whole q-part q^e of #E, times q while that is not yet of order q.  ((#E / q) Q itself is infinity for every Q where the q-part is
    (Z/q)^2 and not cyclic: all of G1's squared primes.)"""
    assert order % q == 0
    for Q in curve_points(cur):
        T = cur.mul(Q, order // q_part(order, q))
        if T is None:
            continue
        while cur.mul(T, q) is not None:
            T = cur.mul(T, q)
        assert cur.is_on_curve(T) and cur.mul(T, q) is None, label
        return T


def point_of_order_q2(cur, order, q, tries=12):
    """a point of order exactly q^2, or None when (#E / q^2) Q has order <= q for the first `tries` curve points Q: the q-part of the
    group is then (Z/q)^2 and not cyclic (a cyclic q-part gives order q^2 with probability 1 - 1/q per try)"""
    if order % (q * q):
        return None
    gen = curve_points(cur)
    for _ in range(tries):
        U = cur.mul(next(gen), order // (q * q))
        if U is not None and cur.mul(U, q) is not None:
            assert cur.mul(U, q * q) is None
            return U
    return None


def cofactor_points():
    z = -o.BLS_X
    h1 = (z - 1) ** 2 // 3
    h2 = (z ** 8 - 4 * z ** 7 + 5 * z ** 6 - 4 * z ** 4 + 6 * z ** 3 - 4 * z ** 2 - 4 * z + 13) // 9
    prod1 = 3
    for q in G1_COFACTOR_PRIMES[1:]:
        prod1 *= q * q
    assert prod1 == h1
    c448 = h2 // (13 ** 2 * 23 ** 2 * 2713 * 11953 * 262069)
    assert c448 * 13 ** 2 * 23 ** 2 * 2713 * 11953 * 262069 == h2 and c448.bit_length() == 448
    out = {}
    for name, cur, enc, h, primes in (("g1", o.G1, pt1, h1, G1_COFACTOR_PRIMES), ("g2", o.G2, pt2, h2, G2_COFACTOR_PRIMES)):
        order = h * o.R
        assert cur.mul(next(curve_points(cur)), order) is None
        S = cur.mul(cur.gen, SUBGROUP_SCALAR)
        recs = []

        def rec(label, order_label, pt):
            assert pt is not None and cur.is_on_curve(pt)
            recs.append({"label": label, "order": order_label, "point": enc(pt), "in_subgroup": cur.in_subgroup(pt)})

        orders = [(q, str(q)) for q in primes] + ([(c448, "c448")] if name == "g2" else [])
        for q, ql in orders:
            T = point_of_order(cur, order, q, ql)
            if name == "g1" and q == 3:
                assert T in ((0, 2), (0, o.P - 2))
                T = (0, 2)                                     # the order-3 point with x = 0: phi fixes it
            rec("T_" + ql, ql, T)
            rec("S+T_" + ql, "r*" + ql, cur.add(S, T))
            rec("-T_" + ql, ql, cur.neg(T))
            if q != c448:
                U = point_of_order_q2(cur, order, q)
                if U is not None:
                    rec("U_%s^2" % ql, ql + "^2", U)
        rec("S", "r", S)
        out[name] = recs
    json.dump(out, open(os.path.join(OUT, "cofactor_points.json"), "w"), indent=0)
    return out


if __name__ == "__main__":
    if sys.argv[1:] == ["cofactor_points"]:
        cofactor_points()
    else:
        main()
