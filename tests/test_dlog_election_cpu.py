"""CPU: the known-discrete-log model of tests/dlog_election.py against the oracle's pairing.  The model is the reference of
tests/test_gpu_verify_dlog.py, so its verdict -- a congruence between integers mod r -- must be the verdict of oracle/pairing.py
groth16_verify and oracle/saver.py verify_encryption, members and sums at infinity included.  Eight instances: the Python pairing is slow."""
import pytest

import bls12_381 as o
import pairing as pg
import saver as sv

import dlog_election as de

R = o.R


@pytest.fixture(scope="module")
def key(cref):
    return de.Key(de.rng(1), 3)


@pytest.fixture(scope="module")
def election(cref):
    return de.Election(de.rng(2), 2, 1)


def oracle_proof_verdict(key, member):
    b = de.proof_batch(key, [member])
    proof = (o.g1_from_limbs(b["A"][0]), o.g2_from_limbs(b["B"][0]), o.g1_from_limbs(b["C"][0]))
    return b["want"][0], int(pg.groth16_verify(key.oracle_vk(), member["xs"], proof))


def oracle_ballot_verdict(el, member):
    b = de.ballot_batch(el, [member])
    proof = (o.g1_from_limbs(b["A"][0]), o.g2_from_limbs(b["B"][0]), o.g1_from_limbs(b["C"][0]))
    ct = [o.g1_from_limbs(row) for row in b["ct"][0]]
    return b["want"][0], int(sv.verify_encryption(el.oracle_pk(), el.key.oracle_vk(), ct, proof, member["xs"]))


def test_an_accepted_proof_and_one_with_z_off_by_one(key):
    rng = de.rng(10)
    xs = [de.nonzero(rng), de.nonzero(rng)]
    assert oracle_proof_verdict(key, de.make_proof(key, xs, rng)) == (1, 1)
    assert oracle_proof_verdict(key, de.make_proof(key, xs, rng, bump=1)) == (0, 0)


def test_an_accepted_proof_whose_accumulated_point_is_infinity(cref):
    rng = de.rng(11)
    g0 = de.nonzero(rng)
    key = de.Key(rng, 3, fixed={0: g0, 1: g0})
    m = de.make_proof(key, [R - 1, 0], rng)
    assert (key.g[0] + (R - 1) * key.g[1]) % R == 0
    assert oracle_proof_verdict(key, m) == (1, 1)


def test_an_accepted_proof_with_a_at_infinity(key):
    rng = de.rng(12)
    m = de.make_proof(key, [de.nonzero(rng), de.nonzero(rng)], rng, s=0)
    assert m["s"] == 0 and not de.proof_batch(key, [m])["A"].any()
    assert oracle_proof_verdict(key, m) == (1, 1)


def _draw(el, rng):
    return [de.nonzero(rng) for _ in range(el.n + 1)], [de.nonzero(rng)]


def _equation_holds(el, m, which):
    """one equation of verify_encryption alone, with the oracle's pairing"""
    b = de.ballot_batch(el, [m])
    ct = [o.g1_from_limbs(row) for row in b["ct"][0]]
    pk, vk = el.oracle_pk(), el.key.oracle_vk()
    if which == 1:
        return pg.pairing_product_is_one([(ct[j], pk["t_g2"][j]) for j in range(el.n + 1)] + [(o.G1.neg(ct[el.n + 1]), o.G2.gen)])
    acc = o.G1.mul(o.G1.gen, el.acc(m["us"], m["xs"]))
    A, B, Cc = o.g1_from_limbs(b["A"][0]), o.g2_from_limbs(b["B"][0]), o.g1_from_limbs(b["C"][0])
    return pg.pairing_product_is_one([(o.G1.neg(A), B), (vk["alpha_g1"], vk["beta_g2"]), (acc, vk["gamma_g2"]), (Cc, vk["delta_g2"])])


def test_an_accepted_ballot(election):
    el, rng = election, de.rng(13)
    assert oracle_ballot_verdict(el, de.make_ballot(el, *_draw(el, rng), rng)) == (0, 1)


def test_a_ballot_failing_only_equation_one(election):
    """the oracle gives one verdict for both equations: it refuses the ballot, and the equation the model calls true holds on its own"""
    el, rng = election, de.rng(15)
    m = de.make_ballot(el, *_draw(el, rng), rng, bump_psi=1)
    assert oracle_ballot_verdict(el, m) == (2, 0)
    assert _equation_holds(el, m, 2)


def test_a_ballot_failing_only_equation_two(election):
    el, rng = election, de.rng(16)
    m = de.make_ballot(el, *_draw(el, rng), rng, bump_z=1)
    assert oracle_ballot_verdict(el, m) == (4, 0)
    assert _equation_holds(el, m, 1)


def test_an_accepted_ballot_with_a_ciphertext_member_at_infinity(election):
    el, rng = election, de.rng(14)
    m = de.make_ballot(el, [de.nonzero(rng), 0, de.nonzero(rng)], [de.nonzero(rng)], rng)
    assert not de.ballot_batch(el, [m])["ct"][0, 1].any()
    assert oracle_ballot_verdict(el, m) == (0, 1)
