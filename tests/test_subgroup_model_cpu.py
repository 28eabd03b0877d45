"""CPU: a plain-integer model of k_subgroup_check's exact ladder (csrc/msm_impl.inc, the group law of csrc/curve.h in XYZZ
coordinates), with a counter per exceptional branch, run over tests/golden/cofactor_points.json: curve points of every small cofactor
order, made by oracle/gen_golden.py cofactor_points().  The yardstick is the oracle's multiplication by r.

What the counters recorded on this fixture (asserted below, so this file is the record):
  G1  every T_q and -T_q (q = 3, 11, 10177, 859267, 52437899: each prime of h1 = (z - 1)^2 / 3 divides z - 1, hence lambda): lambda P = O,
      so t2 ends at infinity and ONLY the kernel's `inf2` term rejects the point (lx = beta x . 0 and ly = y . 0 equal t2.X = t2.Y = 0).
      Every S + T_q, and every G2 point, fails by an honest mismatch, in both coordinates.
  branches (REACHED below).  G1: mixed-add into infinity, equal and opposite, full-add into infinity, equal and opposite, doubling of
      infinity -- T_3 alone meets all seven; T_11 meets mixed-add equal, opposite and full-add equal; the larger primes mixed-add opposite
      only (the closing -P on t2 = P).  G2 (T_13): mixed-add into infinity and opposite, full-add into infinity and opposite, doubling of
      infinity.  Full-add OF infinity is reached by no point: t1 = |z| P is infinity for no point here (|z| is prime to both cofactors'
      small primes).  Small multiples k T_11 and k T_13 were tried and walk the same branches as T_11 and T_13, so the fixture omits them.
  (d) NO fixture point, and no curve point at all, fails in Y only.  Y-only failure means lambda P = -phi(P) != O.  A point with a
      component S != O in the order-r subgroup has lambda P + phi(P) = 2 lambda S + (cofactor part) != O.  A pure cofactor point of prime
      order q has phi(P) = mu P only for mu^2 + mu + 1 = 0 (mod q), and needs lambda = -mu, i.e. lambda^2 - lambda + 1 = 0 (mod q):
      asserted false below for every small prime of both cofactors, and the model finds ex true with ey false on no fixture point
      (the c448 point included).  So `ex`/`ey` independence cannot be pinned from curve points: a kernel that compared X only would
      still differ from this one only on inputs that are not on the curve, which the decoders reject before this kernel runs."""
import os
import re

import pytest

import bls12_381 as o
from conftest import ROOT, dec1, dec2, load_golden

ABS_Z = o.BLS_X
LAMBDA = ABS_Z * ABS_Z - 1
BRANCHES = ("madd_into_inf", "madd_equal", "madd_opposite", "add_into_inf", "add_of_inf", "add_equal", "add_opposite", "dbl_inf")


# ---------------------------------------------------------------------------------------------- the model
class Model:
    """the three group operations as curve.h writes them (EFD dbl-2008-s-1, madd-2008-s, add-2008-s on X, Y, ZZ, ZZZ; infinity <=> ZZ = 0),
    over the oracle's field ops; no inversion anywhere"""

    def __init__(self, F):
        self.F = F
        self.count = dict.fromkeys(BRANCHES, 0)
        self.inf = (F.zero, F.zero, F.zero, F.zero)

    def is_inf(self, a):
        return self.F.is_zero(a[2])

    def dbl(self, a):
        F = self.F
        if self.is_inf(a):
            self.count["dbl_inf"] += 1
            return a
        X, Y, ZZ, ZZZ = a
        U = F.muli(Y, 2)
        V = F.sqr(U)
        W = F.mul(U, V)
        S = F.mul(X, V)
        M = F.muli(F.sqr(X), 3)
        X3 = F.sub(F.sqr(M), F.muli(S, 2))
        Y3 = F.sub(F.mul(M, F.sub(S, X3)), F.mul(W, Y))
        return (X3, Y3, F.mul(V, ZZ), F.mul(W, ZZZ))

    def generic(self, X1, Y1, zz, zzz, Pd, Rd):
        """the common tail of both additions: (X1, Y1) the accumulator scaled to the common denominators zz, zzz before PP, PPP"""
        F = self.F
        PP = F.sqr(Pd)
        PPP = F.mul(Pd, PP)
        Q = F.mul(X1, PP)
        X3 = F.sub(F.sub(F.sqr(Rd), PPP), F.muli(Q, 2))
        Y3 = F.sub(F.mul(Rd, F.sub(Q, X3)), F.mul(Y1, PPP))
        return (X3, Y3, F.mul(zz, PP), F.mul(zzz, PPP))

    def madd(self, a, q, negate=False):
        F = self.F
        qx, qy = q
        if negate:
            qy = F.neg(qy)
        if self.is_inf(a):
            self.count["madd_into_inf"] += 1
            return (qx, qy, F.one, F.one)
        X, Y, ZZ, ZZZ = a
        Pd = F.sub(F.mul(qx, ZZ), X)
        Rd = F.sub(F.mul(qy, ZZZ), Y)
        if F.is_zero(Pd):
            if F.is_zero(Rd):
                self.count["madd_equal"] += 1
                return self.dbl((qx, qy, F.one, F.one))                  # xyzz_dbl_affine: the same formulas at ZZ = ZZZ = 1
            self.count["madd_opposite"] += 1
            return self.inf
        return self.generic(X, Y, ZZ, ZZZ, Pd, Rd)

    def add(self, a, b):
        F = self.F
        if self.is_inf(b):
            self.count["add_of_inf"] += 1
            return a
        if self.is_inf(a):
            self.count["add_into_inf"] += 1
            return b
        U1, U2 = F.mul(a[0], b[2]), F.mul(b[0], a[2])
        S1, S2 = F.mul(a[1], b[3]), F.mul(b[1], a[3])
        Pd, Rd = F.sub(U2, U1), F.sub(S2, S1)
        if F.is_zero(Pd):
            if F.is_zero(Rd):
                self.count["add_equal"] += 1
                return self.dbl(a)
            self.count["add_opposite"] += 1
            return self.inf
        return self.generic(U1, S1, F.mul(a[2], b[2]), F.mul(a[3], b[3]), Pd, Rd)

    def check(self, p, beta):
        """k_subgroup_check on one finite affine point -> dict(inf2, ex, ey, rejected)"""
        F = self.F
        t1 = (p[0], p[1], F.one, F.one)
        for b in range(62, -1, -1):
            t1 = self.dbl(t1)
            if (ABS_Z >> b) & 1:
                t1 = self.madd(t1, p)
        t2 = t1
        for b in range(62, -1, -1):
            t2 = self.dbl(t2)
            if (ABS_Z >> b) & 1:
                t2 = self.add(t2, t1)
        t2 = self.madd(t2, p, negate=True)
        lx = F.mul(F.muli(p[0], beta), t2[2])
        ly = F.mul(p[1], t2[3])
        inf2, ex, ey = self.is_inf(t2), F.eq(lx, t2[0]), F.eq(ly, t2[1])
        return dict(inf2=inf2, ex=ex, ey=ey, rejected=inf2 or not ex or not ey, t2=t2)


def to_affine(F, a):
    if F.is_zero(a[2]):
        return None
    zi = F.inv(a[3])
    z = F.mul(zi, a[2])
    return (F.mul(a[0], F.sqr(z)), F.mul(a[1], zi))


# ---------------------------------------------------------------------------------------------- beta
def cube_roots_of_unity():
    g = next(g for g in range(2, 50) if pow(g, (o.P - 1) // 3, o.P) != 1)
    b = pow(g, (o.P - 1) // 3, o.P)
    assert b != 1 and pow(b, 3, o.P) == 1
    return b, b * b % o.P


def beta_of(cur):
    """the cube root of unity with lambda . generator = (beta x, y)"""
    x, y = cur.mul(cur.gen, LAMBDA)
    assert cur.F.eq(y, cur.gen[1])
    found = [b for b in cube_roots_of_unity() if cur.F.eq(cur.F.muli(cur.gen[0], b), x)]
    assert len(found) == 1
    return found[0]


@pytest.fixture(scope="module")
def betas():
    return {"g1": beta_of(o.G1), "g2": beta_of(o.G2)}


def test_the_two_groups_take_the_two_cube_roots_and_the_kernels_constants_are_these(betas):
    b1, b2 = betas["g1"], betas["g2"]
    assert b1 != b2 and b2 == b1 * b1 % o.P and (b1 * b1 + b1 + 1) % o.P == 0
    assert (LAMBDA * LAMBDA + LAMBDA + 1) % o.R == 0
    src = open(os.path.join(ROOT, "vote_saver_protocol_amd", "csrc", "msm_impl.inc")).read()
    assert int(re.search(r"BLS_ABS_Z = (0x[0-9a-fA-F]+)ULL", src).group(1), 16) == ABS_Z
    consts = re.findall(r"GLV_BETA_MONT\[12\] = \{([^}]*)\}", src)
    assert len(consts) == 2                                                    # VSP_MSM_GROUP == 1, then the other group
    rinv = pow(1 << 384, o.P - 2, o.P)
    for text, want in zip(consts, (b1, b2)):
        words = [int(w.strip().rstrip("u"), 16) for w in text.split(",")]
        mont = sum(w << (32 * i) for i, w in enumerate(words))
        assert len(words) == 12 and mont * rinv % o.P == want


# ---------------------------------------------------------------------------------------------- the fixture through the model
GROUPS = {"g1": (o.G1, dec1), "g2": (o.G2, dec2)}


@pytest.fixture(scope="module")
def runs(betas):
    """group -> [(record, point, model result, branch counts of this point)]"""
    fx = load_golden("cofactor_points.json")
    out = {}
    for name, (cur, dec) in GROUPS.items():
        out[name] = []
        for rec in fx[name]:
            m = Model(cur.F)
            pt = dec(rec["point"])
            out[name].append((rec, pt, m.check(pt, betas[name]), m.count))
    return out


def test_fixture_holds_what_the_generator_promises(runs):
    for name, want_q in (("g1", ("3", "11", "10177", "859267", "52437899")), ("g2", ("13", "23", "2713", "11953", "262069", "c448"))):
        cur = GROUPS[name][0]
        by = {rec["label"]: pt for rec, pt, _, _ in runs[name]}
        S = by["S"]
        assert cur.in_subgroup(S)
        for q in want_q:
            T = by["T_" + q]
            assert cur.is_on_curve(T) and by["-T_" + q] == cur.neg(T) and by["S+T_" + q] == cur.add(S, T)
            if q != "c448":
                assert cur.mul(T, int(q)) is None                              # T != O and q prime: the order is q
        assert all(cur.is_on_curve(pt) for pt in by.values()) and len(by) == len(runs[name])
    assert {rec["label"]: pt for rec, pt, _, _ in runs["g1"]}["T_3"] == (0, 2)


def test_model_verdict_equals_multiplication_by_r(runs, betas):
    for name, (cur, _) in GROUPS.items():
        for rec, pt, res, _ in runs[name]:
            assert cur.in_subgroup(pt) == rec["in_subgroup"], rec["label"]    # the stored verdict is the oracle's
            assert res["rejected"] == (not rec["in_subgroup"]), (name, rec["label"])
            lam = cur.mul(pt, LAMBDA)                                           # and the ladder computes lambda P
            assert to_affine(cur.F, res["t2"]) == lam, (name, rec["label"])
        assert sum(rec["in_subgroup"] for rec, _, _, _ in runs[name]) == 1     # S alone
        for k in (1, 2, 3, o.R - 1, o.R - 2, (o.R - 1) // 2, 0x1234567890ABCDEF, LAMBDA):       # 8 subgroup points
            m = Model(cur.F)
            res = m.check(cur.mul(cur.gen, k), betas[name])
            assert not res["rejected"] and res["ex"] and res["ey"] and not res["inf2"], (name, k)
            assert not any(m.count.values())                                   # a subgroup point meets no exceptional branch


def test_g1_points_of_order_dividing_z_minus_1_are_rejected_by_inf2_alone(runs):
    z = -ABS_Z
    seen = set()
    for rec, pt, res, _ in runs["g1"]:
        q = rec["order"]
        if q.isdigit() and (z - 1) % int(q) == 0:
            assert LAMBDA % int(q) == 0
            assert res["inf2"] and res["ex"] and res["ey"], rec["label"]      # t2 = (0, 0, 0, 0): both compares hold
            seen.add(int(q))
    assert seen == {3, 11, 10177, 859267, 52437899}                           # every prime of h1 = (z - 1)^2 / 3 divides z - 1
    # every G2 prime: lambda P != O, an honest mismatch; so is every S + T_q of either group
    assert [LAMBDA % q for q in (13, 23, 2713, 11953, 262069)] == [2, 17, 384, 4997, 167835]
    for name in ("g1", "g2"):
        for rec, _, res, _ in runs[name]:
            if not rec["in_subgroup"] and not res["inf2"]:
                assert not res["ex"], (name, rec["label"])


REACHED = {
    "g1": {"madd_into_inf", "madd_equal", "madd_opposite", "add_into_inf", "add_equal", "add_opposite", "dbl_inf"},
    "g2": {"madd_into_inf", "madd_opposite", "add_into_inf", "add_opposite", "dbl_inf"},
}


def test_the_fixture_reaches_every_exceptional_branch_of_the_ladder(runs):
    union = {}
    for name in GROUPS:
        total = dict.fromkeys(BRANCHES, 0)
        for _, _, _, count in runs[name]:
            for b in BRANCHES:
                total[b] += count[b]
        union[name] = {b for b in BRANCHES if total[b]}
        print(name, total)
        for rec, _, _, count in runs[name]:
            if any(count.values()):
                print("   ", rec["label"], {b: c for b, c in count.items() if c})
    both = union["g1"] | union["g2"]
    assert {"madd_into_inf", "madd_equal", "madd_opposite", "dbl_inf"} <= both
    assert both & {"add_into_inf", "add_of_inf"}
    assert union == REACHED                                                    # the record: what each group's points reach


def test_no_point_fails_in_y_only(runs):
    for name in GROUPS:
        for rec, _, res, _ in runs[name]:
            assert not (res["ex"] and not res["ey"]), (name, rec["label"])
            if not res["inf2"] and not rec["in_subgroup"]:
                assert not res["ex"] and not res["ey"], (name, rec["label"])   # every honest mismatch shows in both coordinates
    for q in (3, 11, 10177, 859267, 52437899, 13, 23, 2713, 11953, 262069):
        assert (LAMBDA * LAMBDA - LAMBDA + 1) % q != 0                          # no eigenvalue mu of phi on E[q] equals -lambda
