"""The operands and expected values of the tower selftests, shared by the CPU build (test_pairing_cpu.py, g++) and the GPU
(test_gpu_tower.py, vsp_selftest_tower and vsp_selftest_fp2_lanes).  A plain module, computed once per process.

Every expected value comes from the oracle's integers: oracle/pairing.py for Fp12, and for Fp6 and Fp2 the same functions on the value
embedded in Fp12 with the other coefficients zero (the rest of the result is asserted zero here).  The Fp2 inverse is Fp2Ops.inv of
oracle/bls12_381.py, accepted only after f12_mul of the embedded pair gives ONE.  The op codes are those of include/vsp.h."""
import functools

import numpy as np

import bls12_381 as o
import pairing as pg
import wire

P, R = o.P, o.R
HALF = (P + 1) // 2
LEVEL2_OPS = list(range(14))
LEVEL6_OPS = [0, 1, 2, 3, 4, 7, 8]
LEVEL12_OPS = list(range(13))
LANE_OPS = {0: 10, 1: 5}                                            # form -> K, the number of ops (op -1 runs op i mod K on element i)
PAD_SIZES = (65, 127, 130)                                          # a partial last block, and more than two blocks of 64 lanes


def rand_fp(gen):
    a = 0
    for _ in range(6):
        a = (a << 64) | next(gen)
    return a % P


def samples():
    gen = o.splitmix64(381)
    vals = [[rand_fp(gen) for _ in range(12)] for _ in range(16)]
    vals += [pg.ZERO, pg.ONE, pg.W]
    for k in range(12):
        single = [0] * 12
        single[k] = rand_fp(gen)
        vals.append(single)
    return vals


def to_poly(tower):
    """12 tower coefficients (the order of fp12.h) -> the oracle's polynomial in w"""
    return wire.gt_from_tower_le(b"".join(int(x).to_bytes(48, "little") for x in tower))


def to_tower(poly):
    b = wire.gt_to_tower_le(poly)
    return [int.from_bytes(b[48 * i:48 * i + 48], "little") for i in range(12)]


def arr(rows):
    """rows of canonical Fp values -> [n, 6 per value] little-endian uint64 words"""
    n = len(rows)
    flat = b"".join(int(x).to_bytes(48, "little") for row in rows for x in row)
    return np.frombuffer(flat, dtype=np.uint64).reshape(n, -1).copy()


def pad(a, n):
    """the cases repeated up to n rows"""
    reps = -(-n // a.shape[0])
    return np.concatenate([a] * reps)[:n].copy()


# ---- embeddings: Fp6 = the w-free half, Fp2 = coefficient 0
def embed6(t6):
    return to_poly(list(t6) + [0] * 6)


def project6(poly):
    t = to_tower(poly)
    assert not any(t[6:]), "an Fp6 result left Fp6"
    return t[:6]


def embed2(a):
    # wire.gt_from_tower_le for the first coefficient alone: a0 + a1 u = (a0 - a1) + a1 w^6
    poly = [0] * 12
    poly[0], poly[6] = (a[0] - a[1]) % P, a[1] % P
    return poly


def project2(poly):
    assert not any(poly[1:6]) and not any(poly[7:]), "an Fp2 result left Fp2"
    return ((poly[0] + poly[6]) % P, poly[6])


# ---- operands
def fp2_values():
    """the edge values of the Fp2 grid"""
    gen = o.splitmix64(2381)
    r = [rand_fp(gen) for _ in range(5)]
    vals = [(0, 0), (1, 0), (0, 1), (1, 1), (P - 1, 0),
            (P - 1, P - 1), (0, P - 1),
            (r[0], r[0]), (r[1], P - r[1]),                          # c0 = c1, c0 = p - c1
            (r[2], P - r[2]), (r[3], P - 1 - r[3]), (r[4], (P + 1 - r[4]) % P),      # c0 + c1 = p, p - 1, p + 1
            ((P - 1) // 2, (P + 1) // 2)]
    comps = [(1 << 380) - 1] + [1 << (32 * k) for k in range(12)] + [(1 << (32 * k)) - 1 for k in range(1, 12)]
    assert all(0 <= c < P for c in comps)
    vals += [(c, comps[(i + 1) % len(comps)]) for i, c in enumerate(comps)]
    assert all(0 <= x < P and 0 <= y < P for x, y in vals)
    return vals


@functools.lru_cache(maxsize=None)
def fp2_pairs():
    """every pair of the grid and 2 000 random pairs; the count of grid pairs"""
    vals = fp2_values()
    pairs = [(a, b) for a in vals for b in vals]
    grid = len(pairs)
    gen = o.splitmix64(2000)
    for _ in range(2000):
        pairs.append(((rand_fp(gen), rand_fp(gen)), (rand_fp(gen), rand_fp(gen))))
    return pairs, grid


@functools.lru_cache(maxsize=None)
def fp12_values():
    """polynomial form, as samples()"""
    gen = o.splitmix64(12381)
    r = [rand_fp(gen) for _ in range(12)]
    vals = samples()                                                 # 16 random, ZERO, ONE, W, 12 single coefficients
    vals.append(pg.f12_neg(pg.ONE))
    vals.append(to_poly([P - 1] * 12))
    vals.append(to_poly([1] * 12))
    vals.append(to_poly([r[0]] + [0] * 11))                          # in Fp
    vals.append(to_poly(r[:2] + [0] * 10))                           # in Fp2
    vals.append(to_poly(r[:6] + [0] * 6))                            # in Fp6
    vals.append(to_poly([0] * 6 + r[6:]))                            # a pure multiple of w
    vals.append(to_poly([r[k // 2] for k in range(12)]))             # c0 = c1 in every Fp2 coefficient
    vals.append(to_poly([r[k // 2] if k % 2 == 0 else P - r[k // 2] for k in range(12)]))      # c0 = p - c1
    return vals


@functools.lru_cache(maxsize=None)
def fp6_values():
    """tower form, six coefficients: a half of every Fp12 value"""
    out = []
    for v in fp12_values():
        t = to_tower(v)
        out.append(t[:6] if any(t[:6]) else t[6:])
    return out


def partners(vals, zero, one):
    """the operand pairs of the binary ops: every value with itself, ZERO, ONE and the value five places on"""
    A, B = [], []
    for i, a in enumerate(vals):
        for b in (a, zero, one, vals[(i + 5) % len(vals)]):
            A.append(a); B.append(b)
    return A, B


def lines():
    """(l0, l1, l4) as six Fp values: random lines, each one and each two of the three zero, and (1, 0, 0)"""
    gen = o.splitmix64(14)
    out = [[rand_fp(gen) for _ in range(6)] for _ in range(8)]
    for zeros in ((0,), (1,), (2,), (0, 1), (0, 2), (1, 2)):
        l = [rand_fp(gen) for _ in range(6)]
        for z in zeros:
            l[2 * z] = l[2 * z + 1] = 0
        out.append(l)
    out.append([1, 0, 0, 0, 0, 0])
    return out


@functools.lru_cache(maxsize=None)
def final_exp_cases():
    """(f, final_exp(f)): 8 values of which 4 are random, ZERO, two subfield elements (which give ONE) and ONE"""
    v = fp12_values()
    picks = v[:4] + [pg.W, v[19 + 3], to_poly([1] * 12), v[-2]]
    fs = picks + [pg.ZERO, v[-5], v[-4], pg.ONE]                     # v[-5]: in Fp2, v[-4]: in Fp6
    es = [pg.final_exp(f) for f in fs]
    assert es[8] == pg.ZERO and es[9] == pg.ONE and es[10] == pg.ONE and es[11] == pg.ONE
    return fs, es


def cyclotomic_values():
    _, es = final_exp_cases()
    conj = [[(-x) % P if k & 1 else x for k, x in enumerate(e)] for e in es]
    return es + conj


def gt_pow_exponents():
    gen = o.splitmix64(256)
    es = [0, 1, 2, R - 1, R, 1 << 255, (1 << 256) - 1]
    es += [1 << 63, 1 << 64, 1 << 127, 1 << 128, 1 << 191, 1 << 192]
    for _ in range(6):
        e = 0
        for _ in range(4):
            e = (e << 64) | next(gen)
        es.append(e)
    return es


# ---- the tower cases: (level, op) -> (a, b, want) as word arrays of 6 * level columns
def _level12(cases):
    vals = fp12_values()
    T = lambda polys: arr([to_tower(p) for p in polys])
    A, B = partners(vals, pg.ZERO, pg.ONE)
    ta, tb = T(A), T(B)
    cases[12, 0] = (ta, tb, T([pg.f12_mul(a, b) for a, b in zip(A, B)]))
    cases[12, 7] = (ta, tb, T([pg.f12_add(a, b) for a, b in zip(A, B)]))
    cases[12, 8] = (ta, tb, T([pg.f12_sub(a, b) for a, b in zip(A, B)]))
    tv = T(vals)
    cases[12, 1] = (tv, tv, T([pg.f12_mul(a, a) for a in vals]))
    cases[12, 2] = (tv, tv, T([pg.f12_inv(a) if any(a) else pg.ZERO for a in vals]))
    # the conjugation is the Frobenius map p^6, w -> -w in the polynomial form (test_pairing_cpu.py holds it against the oracle's power)
    cases[12, 3] = (tv, tv, T([[(-x) % P if k & 1 else x for k, x in enumerate(a)] for a in vals]))
    f1 = [pg.f12_pow(a, P) for a in vals]
    cases[12, 4] = (tv, tv, T(f1))
    cases[12, 5] = (tv, tv, T([pg.f12_pow(a, P) for a in f1]))
    cyc = cyclotomic_values()
    tc = T(cyc)
    cases[12, 6] = (tc, tc, T([pg.f12_mul(e, e) for e in cyc]))
    fs, es = final_exp_cases()
    cases[12, 9] = (T(fs), T(fs), T(es))
    # the sparse product: every value with every line; the coefficients of b that are no part of the line hold other values
    gen = o.splitmix64(1014)
    A, B, W = [], [], []
    for a in vals:
        for l in lines():
            full = [rand_fp(gen) for _ in range(12)]
            line = [0] * 12
            for t, idx in enumerate((0, 1, 2, 3, 8, 9)):             # tower indices of v^0, v^1 (w^0) and v^1 w
                full[idx] = line[idx] = l[t]
            A.append(to_tower(a)); B.append(full); W.append(to_tower(pg.f12_mul(a, to_poly(line))))
    cases[12, 10] = (arr(A), arr(B), arr(W))
    ones = vals + es
    flags = np.zeros((len(ones), 72), np.uint64)
    flags[:, 0] = [1 if a == pg.ONE else 0 for a in ones]
    assert flags[:, 0].sum() >= 4
    cases[12, 11] = (T(ones), T(ones), flags)
    A, B, W = [], [], []
    for base in es[:2]:
        for e in gt_pow_exponents():
            A.append(to_tower(base))
            B.append([e] + [0] * 11)                                 # e < 2^256 in the first four words; arr() writes 48-byte values
            W.append(to_tower(pg.f12_pow(base, e)))
    cases[12, 12] = (arr(A), arr(B), arr(W))


def _level6(cases):
    vals = fp6_values()
    zero, one = [0] * 6, [1] + [0] * 5
    op6 = lambda f, *xs: project6(f(*[embed6(x) for x in xs]))
    A, B = partners(vals, zero, one)
    ta, tb = arr(A), arr(B)
    cases[6, 0] = (ta, tb, arr([op6(pg.f12_mul, a, b) for a, b in zip(A, B)]))
    cases[6, 7] = (ta, tb, arr([op6(pg.f12_add, a, b) for a, b in zip(A, B)]))
    cases[6, 8] = (ta, tb, arr([op6(pg.f12_sub, a, b) for a, b in zip(A, B)]))
    tv = arr(vals)
    v = [0, 0, 1, 0, 0, 0]
    cases[6, 1] = (tv, tv, arr([op6(pg.f12_mul, a, v) for a in vals]))
    cases[6, 2] = (tv, tv, arr([op6(pg.f12_inv, a) if any(a) else zero for a in vals]))
    # a (b0 + b1 v) and a (b1 v): b0, b1 the first two coefficients of b, the third another value
    W01, W1 = [], []
    for a, b in zip(A, B):
        W01.append(op6(pg.f12_mul, a, list(b[:4]) + [0, 0]))
        W1.append(op6(pg.f12_mul, a, [0, 0] + list(b[2:4]) + [0, 0]))
    cases[6, 3] = (ta, tb, arr(W01))
    cases[6, 4] = (ta, tb, arr(W1))


def _level2(cases):
    pairs, grid = fp2_pairs()
    A, B = [a for a, _ in pairs], [b for _, b in pairs]
    EA, EB = [embed2(a) for a in A], [embed2(b) for b in B]
    ta, tb = arr(A), arr(B)
    put = lambda op, want: cases.__setitem__((2, op), (ta, tb, arr(want)))
    put(0, [project2(pg.f12_mul(a, b)) for a, b in zip(EA, EB)])
    put(1, [project2(pg.f12_mul(a, a)) for a in EA])
    inv = [o.Fp2Ops.inv(a) for a in A]
    for a, ea, i in zip(A, EA, inv):
        assert pg.f12_mul(ea, embed2(i)) == (pg.ONE if any(a) else pg.ZERO)
    put(2, inv)
    put(4, inv)
    conj = [(a[0], (-a[1]) % P) for a in A]
    for k in range(0, grid, 37):                                     # a^p on a few grid values, through the oracle's power
        assert project2(pg.f12_pow(EA[k], P)) == conj[k]
    put(3, conj)
    xi = embed2((1, 1))
    put(5, [project2(pg.f12_mul(a, xi)) for a in EA])
    put(6, [project2(pg.f12_scal(a, HALF)) for a in EA])
    put(7, [project2(pg.f12_add(a, b)) for a, b in zip(EA, EB)])
    put(8, [project2(pg.f12_sub(a, b)) for a, b in zip(EA, EB)])
    put(9, [project2(pg.f12_scal(a, b[0])) for a, b in zip(EA, B)])
    put(10, [project2(pg.f12_neg(a)) for a in EA])
    put(11, [project2(pg.f12_add(a, a)) for a in EA])
    put(12, [(a[0] * HALF % P, a[1] * HALF % P) for a in A])
    put(13, [(pow(a[0], P - 2, P), pow(a[1], P - 2, P)) for a in A])


@functools.lru_cache(maxsize=None)
def tower_cases():
    cases = {}
    _level2(cases)
    _level6(cases)
    _level12(cases)
    assert sorted(cases) == sorted([(2, k) for k in LEVEL2_OPS] + [(6, k) for k in LEVEL6_OPS] + [(12, k) for k in LEVEL12_OPS])
    return cases


# ---- the lane-pair cases: operands a, b, c, d and per (form, op) the expected p and q, in plain integers
@functools.lru_cache(maxsize=None)
def lane_cases():
    pairs, grid = fp2_pairs()
    n = len(pairs)
    quads = []
    for i, (a, b) in enumerate(pairs):
        c, d = pairs[(i + 7) % n]
        quads.append((a, b, c, d))
        if i < grid:                                                 # the two products of a pair share operands
            quads += [(a, b, a, d), (a, b, c, b), (a, b, a, b), (a, b, b, a)]
    if len(quads) % 2 == 0:
        quads.append(quads[grid + 1])
    assert len(quads) % 2 == 1 and len(quads) % 32 != 0
    F = o.Fp2Ops
    A, B, C, D = ([q[k] for q in quads] for k in range(4))
    zero = [(0, 0)] * len(quads)
    ab = [F.mul(a, b) for a, b in zip(A, B)]
    cd = [F.mul(c, d) for c, d in zip(C, D)]
    aa = [F.mul(a, a) for a in A]
    flag = [(1, 1) if a == (0, 0) else (0, 0) for a in A]
    want = {(0, 0): (ab, zero), (0, 1): (aa, zero), (0, 2): (ab, cd),
            (0, 3): ([F.sub(x, y) for x, y in zip(ab, cd)], zero), (0, 4): ([F.add(x, y) for x, y in zip(ab, cd)], zero),
            (0, 5): (flag, zero),
            (0, 6): ([F.add(a, b) for a, b in zip(A, B)], zero), (0, 7): ([F.sub(a, b) for a, b in zip(A, B)], zero),
            (0, 8): ([F.neg(a) for a in A], zero), (0, 9): ([F.add(a, a) for a in A], zero),
            (1, 0): (ab, zero), (1, 1): (ab, zero), (1, 2): (aa, zero), (1, 3): (aa, zero), (1, 4): (aa, zero)}
    for form, K in LANE_OPS.items():                                 # op -1: element i runs op i mod K
        want[form, -1] = tuple([want[form, i % K][side][i] for i in range(len(quads))] for side in (0, 1))
    ops = (arr(A), arr(B), arr(C), arr(D))
    return ops, {key: (arr(p), arr(q)) for key, (p, q) in want.items()}
