"""TEST INFRASTRUCTURE ONLY -- Groth16 keys, proofs, SAVER keys and ballots whose every point is a KNOWN multiple of a generator.

With alpha = a G1, beta = b G2, gamma = c G2, delta = d G2, gamma_ABC[i] = g_i G1 and a proof A = s G1, B = t G2, C = z G1, bilinearity
turns the verification equation into a congruence between integers:

    groth16_verify accepts   <=>   s t = a b + c (g_0 + sum_i x_i g_i) + d z   (mod r)

and, with t_g2[j] = tau_j G2, a ciphertext c_j = u_j G1, psi = psi G1 and the rest inputs x_k:

    equation 1 holds         <=>   sum_{j=0..n} u_j tau_j = psi                                              (mod r)
    equation 2 holds         <=>   s t = a b + c (g_0 + sum_{j=0..n} u_j + sum_k x_k g_{n+1+k}) + d z       (mod r)

so the expected verdict of every member is known without a pairing, and the caller chooses which branch of the public-input
accumulation each member takes (equal points, opposite points, a sum through infinity, members at infinity: the multiple 0).  A point
at infinity pairs to one, which is the multiple 0 in the congruence.  A scalar input that is not below r makes the member malformed.

Python integers and the oracle modules only (the points come from the C oracle's fixed-base multiples of the generators); the library
under test is never called.  tests/test_dlog_election_cpu.py checks the congruences against oracle/pairing.py and oracle/saver.py.
"""
import random

import numpy as np

import bls12_381 as o
import cref
import saver as sv

R = o.R


def _fr(vals):
    return np.array([[(v >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)] for v in vals], dtype=np.uint64).reshape(-1, 4)


def g1_points(scalars):
    """[k G1 for k in scalars] as [n,12] canonical limbs (k = 0: all zero, infinity)"""
    return cref.g1_batch_mul_gen(_fr([k % R for k in scalars])) if len(scalars) else np.zeros((0, 12), np.uint64)


def g2_points(scalars):
    return cref.g2_batch_mul_gen(_fr([k % R for k in scalars])) if len(scalars) else np.zeros((0, 24), np.uint64)


def nonzero(rng):
    return rng.randrange(1, R)


class Key:
    """A Groth16 verification key with known logs.  fixed: {i: g_i} for the gamma_ABC logs the caller chooses; the others are random
    and not zero."""

    def __init__(self, rng, n_abc, fixed=None):
        self.a, self.b, self.c, self.d = (nonzero(rng) for _ in range(4))
        self.g = [nonzero(rng) for _ in range(n_abc)]
        for i, v in (fixed or {}).items():
            self.g[i] = v % R
        self.n_abc = n_abc
        self.alpha = g1_points([self.a])[0]
        self.beta, self.gamma, self.delta = g2_points([self.b, self.c, self.d])
        self.gamma_abc = g1_points(self.g)

    def rhs(self, acc, z):
        """the right side for the log acc of the accumulated public-input point"""
        return (self.a * self.b + self.c * acc + self.d * z) % R

    def oracle_vk(self):
        return dict(alpha_g1=o.g1_from_limbs(self.alpha), beta_g2=o.g2_from_limbs(self.beta), gamma_g2=o.g2_from_limbs(self.gamma),
                    delta_g2=o.g2_from_limbs(self.delta), gamma_ABC_g1=[o.g1_from_limbs(x) for x in self.gamma_abc])


def solve(key, acc, s=None, t=None, z=None, rng=None):
    """(s, t, z) with s t = rhs(acc, z): exactly one of the three may be None and is solved for (t or s must then be invertible, d is);
    with rng, members that are None beyond the first are drawn at random"""
    if rng is not None:
        missing = [k for k, v in (("z", z), ("s", s), ("t", t)) if v is None]
        for k in missing[1:]:
            if k == "s": s = nonzero(rng)
            if k == "t": t = nonzero(rng)
    if z is None:
        z = (s * t - key.a * key.b - key.c * acc) * pow(key.d, -1, R) % R
    elif s is None:
        s = key.rhs(acc, z) * pow(t, -1, R) % R
    elif t is None:
        t = key.rhs(acc, z) * pow(s, -1, R) % R
    return s % R, t % R, z % R


def proof_accepted(key, xs, s, t, z):
    """the model's verdict of the proof (s G1, t G2, z G1) for the public inputs xs (any integers below 2^256)"""
    if any(x >= R for x in xs):
        return False
    acc = (key.g[0] + sum(x * g for x, g in zip(xs, key.g[1:]))) % R
    return (s * t - key.rhs(acc, z)) % R == 0


def make_proof(key, xs, rng, s=None, t=None, z=None, bump=0):
    """a member (xs, s, t, z): the congruence is solved for the one of s, t, z left None (z by default; the scalars enter mod r), then
    bump is added to z.  bump = 0: a true equation; bump = 1: a false one"""
    acc = (key.g[0] + sum((x % R) * g for x, g in zip(xs, key.g[1:]))) % R
    s, t, z = solve(key, acc, s, t, z, rng)
    return dict(xs=list(xs), s=s, t=t, z=(z + bump) % R)


def proof_batch(key, members):
    """-> dict(inputs [n, n_abc - 1, 4] (None when n_abc = 1), A [n,12], B [n,24], C [n,12], want [n] of 0 / 1)"""
    L = key.n_abc - 1
    assert all(len(m["xs"]) == L for m in members)
    inputs = _fr([x for m in members for x in m["xs"]]).reshape(len(members), L, 4) if L else None
    return dict(inputs=inputs, A=g1_points([m["s"] for m in members]), B=g2_points([m["t"] for m in members]), C=g1_points([m["z"] for m in members]),
                want=[int(proof_accepted(key, m["xs"], m["s"], m["t"], m["z"])) for m in members])


class Election:
    """A SAVER election with known logs: a Key of n + 1 + n_rest gamma_ABC points and t_g2[j] = tau_j G2.  The verifier reads t_g2
    alone from the public-key words; the other members are on-curve points of no meaning, at the offsets of oracle/saver.py
    pk_to_words: delta_g1 | delta_s_g1 [n] | t_g1 [n] | t_g2 [n + 1] | delta_sum_s_g1 | gamma_inverse_sum_s_g1."""

    def __init__(self, rng, n, n_rest, fixed=None):
        self.n, self.n_rest = n, n_rest
        self.key = Key(rng, n + 1 + n_rest, fixed)
        self.tau = [nonzero(rng) for _ in range(n + 1)]
        filler = g1_points([nonzero(rng) for _ in range(2 * n + 3)])
        self.pk_words = np.concatenate([filler[:2 * n + 1].reshape(-1), g2_points(self.tau).reshape(-1), filler[2 * n + 1:].reshape(-1)])
        assert self.pk_words.shape[0] == 12 + 24 * n + 24 * (n + 1) + 24

    def oracle_pk(self):
        return sv.pk_from_words(self.pk_words, self.n)

    def acc(self, us, xs):
        k = self.key
        return (k.g[0] + sum(us) + sum((x % R) * g for x, g in zip(xs, k.g[self.n + 1:]))) % R

    def psi(self, us):
        return sum(u * t for u, t in zip(us, self.tau)) % R


def ballot_reason(el, us, psi, xs, s, t, z):
    """the model's reason byte: 1 malformed (a rest scalar not below r), else 2 when equation 1 fails | 4 when equation 2 fails"""
    if any(x >= R for x in xs):
        return 1
    eq1 = (el.psi(us) - psi) % R == 0
    eq2 = (s * t - el.key.rhs(el.acc(us, xs), z)) % R == 0
    return (0 if eq1 else 2) | (0 if eq2 else 4)


def make_ballot(el, us, xs, rng, s=None, t=None, z=None, bump_psi=0, bump_z=0):
    """a ballot (us[0..n], psi, xs, s, t, z): psi and the one of s, t, z left None (z by default) are solved so that both equations
    hold, then bump_psi is added to psi and bump_z to z"""
    assert len(us) == el.n + 1 and len(xs) == el.n_rest
    us = [u % R for u in us]
    s, t, z = solve(el.key, el.acc(us, xs), s, t, z, rng)
    return dict(us=us, psi=(el.psi(us) + bump_psi) % R, xs=list(xs), s=s, t=t, z=(z + bump_z) % R)


def ballot_batch(el, members):
    """-> dict(ct [n, msg_size + 2, 12], rest [n, n_rest, 4] (None when n_rest = 0), A, B, C, want [n] reason bytes)"""
    n, m = el.n, len(members)
    ct = g1_points([k for b in members for k in b["us"] + [b["psi"]]]).reshape(m, n + 2, 12)
    rest = _fr([x for b in members for x in b["xs"]]).reshape(m, el.n_rest, 4) if el.n_rest else None
    return dict(ct=ct, rest=rest, A=g1_points([b["s"] for b in members]), B=g2_points([b["t"] for b in members]), C=g1_points([b["z"] for b in members]),
                want=[ballot_reason(el, b["us"], b["psi"], b["xs"], b["s"], b["t"], b["z"]) for b in members])


def rng(seed):
    return random.Random(seed)
