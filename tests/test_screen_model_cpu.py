"""CPU: the two combined equations of the screened ballot check (include/vsp.h "SAVER ballots screened in bulk") evaluated exactly as
written, in oracle/pairing.py, on elections of known logs (tests/dlog_election.py) with msg_size 1 and two ballots:

    equation 1:  fexp( prod_j ml(S_j, t_g2[j]) * ml(S_psi, -H) ) = 1
    equation 2:  fexp( prod_i ml(z_i A_i, B_i) * ml(ACC, -gamma_g2) * ml(Csum, -delta_g2) * ml(-Z alpha_g1, beta_g2) ) = 1

Each equals one exactly when the integer congruence says so -- sum_i z_i (sum_j u_ij tau_j - psi_i) = 0 and sum_i z_i (s_i t_i - rhs_i)
= 0 mod r -- which pins the signs and the pairing convention before any GPU run.  The Python pairing is slow: four instances."""
import pytest

import bls12_381 as o
import pairing as pg

import dlog_election as de

R = o.R
G1, G2 = o.G1, o.G2


@pytest.fixture(scope="module")
def election(cref):
    return de.Election(de.rng(61), 1, 0)


def combined(el, members, zs):
    """(equation 1 is one, equation 2 is one) from the points of the ballots; (the same from the congruences)"""
    b = de.ballot_batch(el, members)
    n, k = el.n, el.key
    ct = [[o.g1_from_limbs(p) for p in row] for row in b["ct"]]
    A = [o.g1_from_limbs(p) for p in b["A"]]; B = [o.g2_from_limbs(p) for p in b["B"]]; Cc = [o.g1_from_limbs(p) for p in b["C"]]
    gabc = [o.g1_from_limbs(p) for p in k.gamma_abc]
    t_g2 = [o.g2_from_limbs(p) for p in de.g2_points(el.tau)]

    def lincomb(points):
        s = None
        for z, p in zip(zs, points):
            s = G1.add(s, G1.mul(p, z))
        return s

    def acc(i):
        s = gabc[0]
        for j in range(n + 1):
            s = G1.add(s, ct[i][j])
        return s
    f = pg.ONE
    for j in range(n + 1):
        f = pg.f12_mul(f, pg.miller_loop(t_g2[j], lincomb([c[j] for c in ct])))
    f = pg.f12_mul(f, pg.miller_loop(G2.neg(G2.gen), lincomb([c[n + 1] for c in ct])))
    eq1 = pg.final_exp(f) == pg.ONE
    f = pg.ONE
    for z, a, bb in zip(zs, A, B):
        f = pg.f12_mul(f, pg.miller_loop(bb, G1.mul(a, z)))
    f = pg.f12_mul(f, pg.miller_loop(G2.neg(o.g2_from_limbs(k.gamma)), lincomb([acc(i) for i in range(len(members))])))
    f = pg.f12_mul(f, pg.miller_loop(G2.neg(o.g2_from_limbs(k.delta)), lincomb(Cc)))
    Z = sum(zs) % R
    f = pg.f12_mul(f, pg.miller_loop(o.g2_from_limbs(k.beta), G1.neg(G1.mul(o.g1_from_limbs(k.alpha), Z))))
    eq2 = pg.final_exp(f) == pg.ONE
    c1 = sum(z * (el.psi(m["us"]) - m["psi"]) for z, m in zip(zs, members)) % R == 0
    c2 = sum(z * (m["s"] * m["t"] - k.rhs(el.acc(m["us"], m["xs"]), m["z"])) for z, m in zip(zs, members)) % R == 0
    return (eq1, eq2), (c1, c2)


def ballot(el, rng, **kw):
    return de.make_ballot(el, [de.nonzero(rng) for _ in range(el.n + 1)], [], rng, **kw)


def coefficients(rng):
    return [rng.randrange(1, 1 << 128) for _ in range(2)]


def test_two_valid_ballots_satisfy_both_combined_equations(election):
    rng = de.rng(62)
    got, want = combined(election, [ballot(election, rng), ballot(election, rng)], [1, (1 << 128) - 1])
    assert got == want == (True, True)


def test_one_bad_ballot_fails_the_equation_it_fails_alone(election):
    rng = de.rng(63)
    got, want = combined(election, [ballot(election, rng, bump_psi=1), ballot(election, rng)], coefficients(rng))
    assert got == want == (False, True)
    got, want = combined(election, [ballot(election, rng), ballot(election, rng, bump_z=1)], coefficients(rng))
    assert got == want == (True, False)


def test_a_cancelling_pair_passes_under_its_coefficients_and_fails_when_they_are_swapped(election):
    """defects z_2 and -z_1 in psi and in z: under (z_1, z_2) both equations hold although neither ballot is valid -- coefficients known
    to the sender protect nothing"""
    rng = de.rng(64)
    z1, z2 = coefficients(rng)
    pair = [ballot(election, rng, bump_psi=z2, bump_z=z2), ballot(election, rng, bump_psi=R - z1, bump_z=R - z1)]
    assert [de.ballot_reason(election, m["us"], m["psi"], m["xs"], m["s"], m["t"], m["z"]) for m in pair] == [6, 6]
    got, want = combined(election, pair, [z1, z2])
    assert got == want == (True, True)
    got, want = combined(election, pair, [z2, z1])
    assert got == want == (False, False)
