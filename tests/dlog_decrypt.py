"""TEST INFRASTRUCTURE ONLY -- SAVER decryption keys and ciphertexts whose every point is a KNOWN multiple of a generator, in the
style of tests/dlog_election.py (whose point helpers this file uses).

With G_i = g_i G1, V_i = a_i G2, W_i = b_i G2 (i = 1..n), rho_g2 = rho G2, a ciphertext c_j = u_j G1 and a stated proof nu = nu G1,
bilinearity turns the equations of decrypt and verify_decryption into congruences between integers (logs to the base e(G1, G2)):

    value_i = base_i^m       <=>   u_i b_i - nu a_i = m g_i b_i                 (mod r)        nu = rho u_0 in decrypt
    equation 0 holds         <=>   nu = rho u_0                                  (mod r)

so   u_i = (m_i g_i b_i + rho u_0 a_i) / b_i   makes c_i decrypt to m_i for ANY m_i, at no pairing's cost, and the slot logarithm of an
arbitrary ciphertext is  (u_i b_i - rho u_0 a_i) / (g_i b_i).  A point at infinity is the multiple 0.

Python integers and the oracle modules only; the library under test is never called."""
import numpy as np

import bls12_381 as o
from dlog_election import R, _fr, g1_points, g2_points, nonzero

NONE = (1 << 64) - 1


class DecryptKey:
    """logs g[0..n] (g[0] is the constant term's, unused by decryption), a[i], b[i] for slot i = 0..n-1, rho; gamma_abc [n+1,12] and
    vk_words in the layout of oracle/saver.py vk_to_words: rho_g2 | rho_sv_g2 [n] | rho_rhov_g2 [n]"""

    def __init__(self, rng, n):
        self.n = n
        self.g = [nonzero(rng) for _ in range(n + 1)]
        self.a = [nonzero(rng) for _ in range(n)]
        self.b = [nonzero(rng) for _ in range(n)]
        self.rho = nonzero(rng)
        self.gamma_abc = g1_points(self.g)
        self.vk_words = g2_points([self.rho] + self.a + self.b).reshape(-1)
        self.rho_limbs = _fr([self.rho])[0]

    def oracle_vk(self):
        import saver as sv
        return sv.vk_from_words(self.vk_words, self.n)

    def oracle_gamma_abc(self):
        return [o.g1_from_limbs(x) for x in self.gamma_abc]

    def member(self, i, m, u0):
        """u_{i+1} for slot i to hold m (any integer, taken mod r) beside c_0 = u0 G1"""
        return ((m % R) * self.g[i + 1] * self.b[i] + self.rho * u0 * self.a[i]) * pow(self.b[i], -1, R) % R

    def ciphertext(self, msgs, rng, u0=None, psi=None):
        """the logs u_0 .. u_n, psi of a ciphertext that decrypts to msgs (psi takes no part in decryption: random)"""
        u0 = nonzero(rng) if u0 is None else u0 % R
        return [u0] + [self.member(i, m, u0) for i, m in enumerate(msgs)] + [nonzero(rng) if psi is None else psi]

    def slot_log(self, us, i, nu=None):
        """the m mod r with value_i = base_i^m for the ciphertext logs us and the proof log nu (default: the true rho u_0)"""
        nu = self.rho * us[0] % R if nu is None else nu % R
        return (us[i + 1] * self.b[i] - nu * self.a[i]) * pow(self.g[i + 1] * self.b[i], -1, R) % R

    def decrypt(self, us, max_value):
        """the model's (msgs, status) of one ciphertext"""
        logs = [self.slot_log(us, i) for i in range(self.n)]
        return [m if m <= max_value else NONE for m in logs], [0 if m <= max_value else 1 for m in logs]

    def reason(self, us, msgs, nu):
        """the model's (reason, first_bad_slot) of a stated result: msgs any integers below 2^256, nu the log of the stated proof"""
        if any(m >= R for m in msgs):
            return 1, 0xFFFFFFFF
        bad = [i for i in range(self.n) if self.slot_log(us, i, nu) != msgs[i]]
        eq0 = (nu - self.rho * us[0]) % R == 0
        return (0 if eq0 else 2) | (4 if bad else 0), bad[0] if bad else 0xFFFFFFFF


def ct_batch(key, members):
    """ciphertext logs (n + 2 each) -> [count, n + 2, 12] canonical limbs"""
    return g1_points([u for us in members for u in us]).reshape(len(members), key.n + 2, 12)


def scalars(msgs):
    """[count][n] integers below 2^256 -> [count, n, 4] limbs (not reduced: a value >= r stays what it is)"""
    return np.array([[[(m >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)] for m in row] for row in msgs], dtype=np.uint64)
