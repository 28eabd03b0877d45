"""Big-integer model of Jubjub, its Pedersen hash and the registry tree: what the GPU kernels and csrc/jubjub.h are compared with, bit
for bit.  Test infrastructure (beside dlog_election.py), written from the definitions of the issue / DESIGN.md 3.6i alone.

Two routes to a hash, which the CPU test holds against each other:
    hash_definition   sum_i [<M_i>] G_i by affine double-and-add over the integer <M_i> = sum_j enc(chunk) 2^(4 j)   (~70 ms at 510 bits)
    hash_windowed     one extended-coordinate addition per chunk from a table of k 2^(4 j) G_i                      (~1 ms)
Generators come from SHA-256 try-and-increment on v, multiplied by the cofactor 8 and checked to have order s."""
import hashlib

R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
D = (-10240 * pow(10241, -1, R)) % R
S = 6554484396890773809930967563523245729705921265872317281365359162392183254199
IDENTITY = (0, 1)
WINDOWS, SEGMENT_BITS, DIGEST_BITS = 63, 189, 255

assert D == 0x2a9318e74bfa2b48f5fd9207e6bd7fd4292d7f6d37579d2601065fd6d6343eb1
assert pow(R - 1, (R - 1) // 2, R) == 1 and pow(D, (R - 1) // 2, R) == R - 1      # -1 is a square, d is not: the addition law is complete


# ---- affine arithmetic: the definition
def on_curve(p):
    u, v = p
    return (v * v - u * u - 1 - D * u * u % R * v * v) % R == 0


def add(p, q):
    (u1, v1), (u2, v2) = p, q
    t = D * u1 % R * u2 % R * v1 % R * v2 % R
    return ((u1 * v2 + v1 * u2) * pow(1 + t, -1, R) % R, (v1 * v2 + u1 * u2) * pow(1 - t, -1, R) % R)


def neg(p):
    return ((-p[0]) % R, p[1])


def mul(p, k):
    acc, base = IDENTITY, p
    while k:
        if k & 1:
            acc = add(acc, base)
        base = add(base, base)
        k >>= 1
    return acc


def has_order_s(p):
    return on_curve(p) and p != IDENTITY and mul(p, S) == IDENTITY


def sqrt_mod(a):
    """a square root of a mod R, or None (Tonelli-Shanks: R - 1 = 2^32 q)"""
    a %= R
    if a == 0:
        return 0
    if pow(a, (R - 1) // 2, R) != 1:
        return None
    q, e = R - 1, 0
    while q % 2 == 0:
        q //= 2; e += 1
    z = 2
    while pow(z, (R - 1) // 2, R) == 1:
        z += 1
    m, c, t, x = e, pow(z, q, R), pow(a, q, R), pow(a, (q + 1) // 2, R)
    while t != 1:
        i, t2 = 0, t
        while t2 != 1:
            t2 = t2 * t2 % R; i += 1
        b = pow(c, 1 << (m - i - 1), R)
        m, c = i, b * b % R
        t, x = t * c % R, x * b % R
    return x


def raw_point(tag, index):
    """a point of the curve from SHA-256(tag | index | counter) taken as v: NOT cleared of the cofactor (its order divides 8 s)"""
    counter = 0
    while True:
        v = int.from_bytes(hashlib.sha256(b"%s|%d|%d" % (tag, index, counter)).digest(), "big") % R
        counter += 1
        den = (1 + D * v * v) % R
        u = sqrt_mod((v * v - 1) * pow(den, -1, R))
        if u is None or (u, v) == IDENTITY:
            continue
        p = (u, v)
        assert on_curve(p)
        return p


def generator(tag, index):
    while True:
        g = mul(raw_point(tag, index), 8)
        if g != IDENTITY:
            assert has_order_s(g)
            return g
        index += 1 << 20


def generators(count, tag=b"vsp-test-pedersen"):
    return [generator(tag, i) for i in range(count)]


def uncleared_point(tag=b"vsp-test-uncleared"):
    """a curve point outside the prime-order subgroup"""
    i = 0
    while True:
        p = raw_point(tag, i)
        if mul(p, S) != IDENTITY:
            return p
        i += 1


# ---- messages: a list of bits, bit k first
def bits_of(value, n):
    return [(value >> k) & 1 for k in range(n)]


def chunks_of(bits):
    padded = list(bits) + [0] * (-len(bits) % 3)
    return [(padded[i], padded[i + 1], padded[i + 2]) for i in range(0, len(padded), 3)]


def encode(chunk):
    s0, s1, s2 = chunk
    return (1 - 2 * s2) * (1 + s0 + 2 * s1)


def schedule(nbits):
    """(segment, window) of every chunk of a message of nbits bits"""
    return [(c // WINDOWS, c % WINDOWS) for c in range((nbits + 2) // 3)]


def hash_definition(gens, bits):
    assert 1 <= len(bits) <= SEGMENT_BITS * len(gens)
    scalars = {}
    for c, chunk in enumerate(chunks_of(bits)):
        scalars[c // WINDOWS] = scalars.get(c // WINDOWS, 0) + encode(chunk) * (1 << (4 * (c % WINDOWS)))
    acc = IDENTITY
    for i, m in sorted(scalars.items()):
        acc = add(acc, mul(gens[i], m % S))
    return acc


# ---- the windowed route: extended coordinates, a = -1
def ext_add(p, q):
    X1, Y1, Z1, T1 = p
    X2, Y2, Z2, T2 = q
    A = (Y1 - X1) * (Y2 - X2) % R; B = (Y1 + X1) * (Y2 + X2) % R
    C = T1 * 2 * D % R * T2 % R; Dd = 2 * Z1 * Z2 % R
    E, F, G, H = B - A, Dd - C, Dd + C, B + A
    return (E * F % R, G * H % R, F * G % R, E * H % R)


def ext_of(p):
    return (p[0], p[1], 1, p[0] * p[1] % R)


def affine_of(e):
    zi = pow(e[2], -1, R)
    return (e[0] * zi % R, e[1] * zi % R)


class Table:
    """k 2^(4 j) G_i for every generator, window and k = 1 .. 4 (extended, Z = 1)"""

    def __init__(self, gens):
        self.gens = list(gens)
        self.rows = []
        for g in self.gens:
            base = g
            for _ in range(WINDOWS):
                two = add(base, base); four = add(two, two)
                self.rows.append([ext_of(base), ext_of(two), ext_of(add(two, base)), ext_of(four)])
                base = add(four, four); base = add(base, base)

    def hash_point(self, bits):
        assert 1 <= len(bits) <= SEGMENT_BITS * len(self.gens)
        acc = (0, 1, 1, 0)
        for c, (s0, s1, s2) in enumerate(chunks_of(bits)):
            X, Y, Z, T = self.rows[c][s0 + 2 * s1]
            acc = ext_add(acc, ((-X) % R, Y, Z, (-T) % R) if s2 else (X, Y, Z, T))
        return affine_of(acc)

    def hash(self, bits):
        return self.hash_point(bits)[0]

    # ---- the tree: levels[l][i], level 0 the leaves
    def tree(self, pks, depth, hash_leaves=True):
        keys = list(pks) + [0] * ((1 << depth) - len(pks))
        assert len(keys) == 1 << depth and all(k >> DIGEST_BITS == 0 for k in keys)
        memo = {}

        def h(bits_key, bits):
            if bits_key not in memo:
                memo[bits_key] = self.hash(bits)
            return memo[bits_key]
        level = [h(("leaf", k), bits_of(k, DIGEST_BITS)) for k in keys] if hash_leaves else keys
        levels = [level]
        for _ in range(depth):
            level = [h((level[2 * i], level[2 * i + 1]), bits_of(level[2 * i], DIGEST_BITS) + bits_of(level[2 * i + 1], DIGEST_BITS)) for i in range(len(level) // 2)]
            levels.append(level)
        return levels


def copath(levels, x):
    return [levels[l][(x >> l) ^ 1] for l in range(len(levels) - 1)]


def rt_scalars(root):
    return [root & ((1 << 254) - 1), root >> 254]


def node_blob(digest):
    out = bytearray(32)
    for b in range(DIGEST_BITS):
        if (digest >> b) & 1:
            out[b // 8] |= 1 << (7 - b % 8)
    return bytes(out)


def tree_blob(levels):
    return b"".join(node_blob(n) for level in levels for n in level)


# ---- the C ABI's layouts
def words(value, n=4):
    return [(value >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(n)]


def point_words(p):
    return words(p[0]) + words(p[1])


def message_words(bits):
    value = sum(b << k for k, b in enumerate(bits))
    return words(value, (len(bits) + 63) // 64)
