"""GPU: vsp_groth16_verify_batch, vsp_saver_verify_batch and vsp_multi_pairing_batch on keys, proofs and ballots made of KNOWN multiples
of the generators (tests/dlog_election.py; its verdicts are checked against the oracle's pairing in tests/test_dlog_election_cpu.py).
The expected verdict of every member is a congruence between integers, so the members are chosen to drive the public-input accumulation
of k_verify_prepare / k_ballot_prepare into its exceptional branches -- equal points with an affine and with a non-affine accumulator,
opposite points, a sum carried through infinity and out of it again, the final addition of gamma_ABC[0] meeting an equal or the opposite
point -- which proofs of the library's own prover over a random key never reach; `walk` below replays the kernels' order of additions
on the logs and the tests assert that the branch each case is named after is taken.  Special members sit at lanes 0, 63, 64, 65 and in
between, among ordinary accepted and rejected ones.  Shapes: n_abc 1 and 41, batch sizes around the block edge, every piece size;
products of 4 to 1024 pairs (the 2^16-pair cap of a piece); msg_size 1 .. 64 and 1022 in every grouping, with and without rest inputs."""
import numpy as np
import pytest

import bls12_381 as o
import pairing as pg
import wire

import dlog_election as de

import vote_saver_protocol_amd as v

pytestmark = pytest.mark.gpu
R = o.R
CHUNKS = [None, 1, 20]                                              # option "pairing_chunk": its default, one member a piece, 20
SLOTS = [0, 63, 64, 65] + list(range(1, 63, 2)) + list(range(2, 63, 2))      # where the special members of a batch go, in this order


def walk(gx, tail):
    """The accumulation of k_verify_prepare / k_ballot_prepare replayed on logs: from infinity, 64 windows of 4 bits from the top (four
    doublings, then digit * g_i for every (g_i, x_i) of gx in order), then the logs of `tail` one by one; every addition as xyzz_madd
    branches.  -> (the set of branches taken, the log of the sum or None for infinity)"""
    acc, affine, ev = None, False, set()

    def add(q):
        nonlocal acc, affine
        q %= R
        if q == 0:
            return
        if acc is None:
            if "opposite" in ev:
                ev.add("left infinity again")
            acc, affine = q, True
        elif acc == q:
            ev.add("equal, affine accumulator" if affine else "equal, ZZ != 1")
            acc, affine = 2 * q % R, False
        elif (acc + q) % R == 0:
            ev.add("opposite")
            acc = None
        else:
            acc, affine = (acc + q) % R, False

    for w in range(63, -1, -1):
        if w != 63:
            if acc is None and "opposite" in ev:
                ev.add("infinity doubled")
            if acc is not None:
                acc, affine = 16 * acc % R, False
        for g, x in gx:
            add(((x >> (4 * w)) & 15) * g)
    for q in tail:
        add(q)
    return ev, acc


def place(specials, size, filler):
    assert len(specials) <= len(SLOTS) and size > 65
    out = [None] * size
    for slot, m in zip(SLOTS, specials):
        out[slot] = m
    return [filler(i) if m is None else m for i, m in enumerate(out)]


def with_option(ctx, name, value, default, fn):
    if value is None:
        return fn()
    ctx.set_option(name, value)
    try:
        return fn()
    finally:
        ctx.set_option(name, default)


# ------------------------------------------------------------------------------------------------------------------- Groth16
def g16_batch(ctx, seed, fixed, cases, size=66, n_abc=4):
    """cases: (xs, the branches the accumulation must take, make_proof keywords); each becomes an accepted and a rejected (z + 1) member.
    fixed: a function of the rng giving the chosen gamma_ABC logs"""
    rng = de.rng(seed)
    key = de.Key(rng, n_abc, fixed(rng) if fixed else None)
    specials = []
    for xs, branches, kw in cases:
        xs = xs(rng, key) if callable(xs) else xs
        ev, acc = walk(list(zip(key.g[1:], xs)), [key.g[0]])
        assert branches <= ev, (branches, ev)
        assert (acc or 0) == (key.g[0] + sum(x * g for x, g in zip(xs, key.g[1:]))) % R
        for bump in (0, 1):
            m = de.make_proof(key, xs, rng, bump=bump, **kw)
            assert de.proof_accepted(key, m["xs"], m["s"], m["t"], m["z"]) == (bump == 0)
            specials.append(m)
    filler = lambda i: de.make_proof(key, [rng.randrange(R) for _ in range(n_abc - 1)], rng, bump=int(i % 3 == 1))
    b = de.proof_batch(key, place(specials, size, filler))
    assert 0 < sum(b["want"]) < size
    vk = v.VerifyingKey(ctx, key.alpha, key.beta, key.gamma, key.delta, key.gamma_abc)
    assert vk.n_abc == n_abc
    return vk, b, key


def g16_equal_first(ctx):
    """g_2 = g_1 and x_1 = x_2: in the first window with a digit the accumulator is the affine d G_1 when the equal d G_2 arrives"""
    def fixed(rng):
        g1 = de.nonzero(rng)
        return {1: g1, 2: g1}
    same = lambda rng, key: [x := de.nonzero(rng), x, rng.randrange(R)]
    return g16_batch(ctx, 101, fixed, [(same, {"equal, affine accumulator"}, {}), ([5, 5, 0], {"equal, affine accumulator"}, {})])


def g16_equal_later(ctx):
    """g_2 = 16 g_1, x_1 = 0x10 16^w, x_2 = 16^w: G_1 enters at window w + 1, is doubled four times, and meets 16 G_1 = G_2 at window w
    with ZZ != 1 (x_3 has no digit above window w: it is added after x_2)"""
    def fixed(rng):
        g1 = de.nonzero(rng)
        return {1: g1, 2: 16 * g1}
    case = lambda w: (lambda rng, key: [0x10 << (4 * w), 1 << (4 * w), rng.randrange(16 ** (w + 1))], {"equal, ZZ != 1"}, {})
    return g16_batch(ctx, 102, fixed, [case(0), case(31), case(62)])


def g16_opposite(ctx):
    """g_2 = r - g_1 and x_1 = x_2: the sum becomes infinity in every window and is doubled on; with x_3 it leaves infinity again"""
    def fixed(rng):
        g1 = de.nonzero(rng)
        return {1: g1, 2: R - g1}
    full = lambda rng: rng.randrange(R // 2, R)                    # a digit in the top window
    return g16_batch(ctx, 103, fixed, [(lambda rng, key: [x := full(rng), x, 0], {"opposite", "infinity doubled"}, {}),
                                       (lambda rng, key: [x := full(rng), x, full(rng)], {"opposite", "left infinity again"}, {})])


def g16_zero_inputs(ctx):
    """every input zero: the sum is G_0 alone"""
    return g16_batch(ctx, 104, None, [([0, 0, 0], set(), {})])


def g16_final_g0(ctx):
    """the final addition of G_0: g_1 = g_0 with x_1 = 1 (equal, affine), 16 g_2 = g_0 with x_2 = 0x10 (equal, ZZ != 1), x_1 = r - 1
    (opposite: the pair (acc, -gamma) contributes one)"""
    def fixed(rng):
        g0 = 16 * de.nonzero(rng) % R
        return {0: g0, 1: g0, 2: g0 * pow(16, -1, R)}
    return g16_batch(ctx, 105, fixed, [([1, 0, 0], {"equal, affine accumulator"}, {}), ([0, 0x10, 0], {"equal, ZZ != 1"}, {}), ([R - 1, 0, 0], {"opposite"}, {})])


def g16_infinity(ctx):
    """A, B or C at infinity with a true equation (and, one line on, a false one)"""
    rnd = lambda rng, key: [rng.randrange(R) for _ in range(3)]
    return g16_batch(ctx, 106, None, [(rnd, set(), dict(s=0)), (rnd, set(), dict(t=0)), (rnd, set(), dict(z=0))])


SCALARS = [0, 1, R - 1, (R - 1) // 2, 1 << 254] + [15 * 16 ** w for w in range(63)] + [7 * 16 ** 63]


def g16_scalars(ctx):
    """x_1 over the edge scalars (accepted), a few of them rejected, and scalars not below r, which are rejected although z solves the
    equation for x mod r"""
    rng = de.rng(107)
    key = de.Key(rng, 4)
    assert all(x < R for x in SCALARS) and len(SCALARS) == 69
    ms = [de.make_proof(key, [x, rng.randrange(R), rng.randrange(R)], rng, bump=int(i % 8 == 3)) for i, x in enumerate(SCALARS)]
    ms += [de.make_proof(key, xs, rng) for xs in ([R, 1, 2], [3, R + 1, 4], [5, 6, (1 << 256) - 1], [rng.randrange((1 << 256) - R) + R, 0, 0])]
    while len(ms) < 129:
        ms.append(de.make_proof(key, [rng.randrange(R) for _ in range(3)], rng, bump=int(len(ms) % 3 == 1)))
    ms[0], ms[69] = ms[69], ms[0]                                    # a scalar not below r at lane 0
    ms[64], ms[70] = ms[70], ms[64]
    b = de.proof_batch(key, ms)
    assert [b["want"][k] for k in (0, 64, 71, 72)] == [0, 0, 0, 0]
    return v.VerifyingKey(ctx, key.alpha, key.beta, key.gamma, key.delta, key.gamma_abc), b, key


def g16_no_inputs(ctx):
    """n_abc = 1: no public input, the sum is G_0"""
    rng = de.rng(108)
    key = de.Key(rng, 1)
    b = de.proof_batch(key, [de.make_proof(key, [], rng, bump=int(i in (0, 62, 64, 128) or i % 5 == 2)) for i in range(129)])
    assert b["inputs"] is None
    return v.VerifyingKey(ctx, key.alpha, key.beta, key.gamma, key.delta, key.gamma_abc), b, key


def g16_forty_inputs(ctx):
    return g16_batch(ctx, 109, None, [(lambda rng, key: [rng.randrange(R) for _ in range(40)], set(), {}), ([0] * 39 + [R - 1], set(), {})], n_abc=41)


G16 = dict(equal_first=g16_equal_first, equal_later=g16_equal_later, opposite=g16_opposite, zero_inputs=g16_zero_inputs, final_g0=g16_final_g0,
           infinity=g16_infinity, scalars=g16_scalars, no_inputs=g16_no_inputs, forty_inputs=g16_forty_inputs)


@pytest.fixture(scope="module")
def g16(ctx, cref):
    made = {}

    def get(name):
        if name not in made:
            made[name] = G16[name](ctx)
        return made[name]
    yield get
    for vk, _, _ in made.values():
        vk.free()


def g16_verdicts(ctx, vk, b, chunk, sl=slice(None)):
    inputs = None if b["inputs"] is None else b["inputs"][sl]
    return with_option(ctx, "pairing_chunk", chunk, 1 << 14, lambda: v.groth16_verify_batch(ctx, vk, inputs, b["A"][sl], b["B"][sl], b["C"][sl]).tolist())


@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("name", list(G16))
def test_groth16_verdicts_are_the_models(ctx, g16, name, chunk):
    vk, b, _ = g16(name)
    assert g16_verdicts(ctx, vk, b, chunk) == b["want"]


@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("size", [1, 63, 64, 65])
@pytest.mark.parametrize("name", ["no_inputs", "scalars"])
def test_groth16_batch_sizes(ctx, g16, name, size, chunk):
    """parts of the two batches of 129, which test_groth16_verdicts_are_the_models runs whole"""
    vk, b, _ = g16(name)
    sl = slice(129 - size, 129) if size < 64 else slice(0, size)
    assert g16_verdicts(ctx, vk, b, chunk, sl) == b["want"][sl]


# ------------------------------------------------------------------------------------------------------- products of pairings
@pytest.fixture(scope="module")
def gt_values():
    """ONE, e(G1, G2) and its square: the three oracle values every expected product is one of"""
    e = pg.final_exp(pg.miller_loop(o.G2.gen, o.G1.gen))
    return [wire.gt_to_tower_le(x) for x in (pg.ONE, e, pg.f12_mul(e, e))]


@pytest.fixture(scope="module")
def pool(cref):
    rng = de.rng(201)
    ab = [(de.nonzero(rng), de.nonzero(rng)) for _ in range(64)]
    return dict(ab=ab, g1=de.g1_points([a for a, _ in ab]), g2=de.g2_points([b for _, b in ab]))


def products(pool, m, n, seed):
    """n products of m pairs from the pool; the last pair of product k makes the exponent sum k mod 3.  Product 1 (and every tenth after)
    has an infinity G1 member, product 2 (and every tenth after) an infinity G2 member, whose pairs count as one"""
    rng = de.rng(seed)
    idx = np.array([[rng.randrange(64) for _ in range(m - 1)] for _ in range(n)]).reshape(n, m - 1)
    g1 = np.zeros((n, m, 12), np.uint64); g2 = np.zeros((n, m, 24), np.uint64)
    g1[:, :m - 1] = pool["g1"][idx]; g2[:, :m - 1] = pool["g2"][idx]
    last_a, last_b = [], []
    for k in range(n):
        e = [pool["ab"][i][0] * pool["ab"][i][1] for i in idx[k]]
        at = (m - 1) // 2
        if k % 10 == 1:
            g1[k, at] = 0; e[at] = 0
        if k % 10 == 2:
            g2[k, at] = 0; e[at] = 0
        b = de.nonzero(rng)
        last_a.append((k % 3 - sum(e)) * pow(b, -1, R) % R); last_b.append(b)
    g1[:, m - 1] = de.g1_points(last_a); g2[:, m - 1] = de.g2_points(last_b)
    return g1.reshape(n * m, 12), g2.reshape(n * m, 24), [k % 3 for k in range(n)]


@pytest.mark.parametrize("m,n", [(4, 7), (7, 6), (64, 6), (65, 5), (1024, 65)])
def test_products_of_many_pairings(ctx, pool, gt_values, m, n):
    """m = 1024, n = 65: 66 560 pairs, above the 2^16 of a piece, so the work is cut into pieces of 64 products and one"""
    g1, g2, want = products(pool, m, n, 210 + m)
    gt, is_one = v.multi_pairing_batch(ctx, g1, g2, m)
    assert is_one.tolist() == [int(e == 0) for e in want]
    for k in range(n):
        assert gt[k].tobytes() == gt_values[want[k]], k


# ------------------------------------------------------------------------------------------------------------------------ SAVER
def saver_reasons(ctx, ver, b, sl=slice(None)):
    rest = None if b["rest"] is None else b["rest"][sl]
    verdict, reason = v.saver_verify_batch(ctx, ver, b["ct"][sl], rest, b["A"][sl], b["B"][sl], b["C"][sl])
    assert verdict.tolist() == [int(r == 0) for r in reason]
    return reason.tolist()


def make_verifier(ctx, el):
    k = el.key
    ver = v.SaverVerifier(ctx, el.pk_words, k.alpha, k.beta, k.gamma, k.delta, k.gamma_abc, el.n)
    assert ver.n_abc == el.n + 1 + el.n_rest
    return ver


def ordinary_ballot(el, rng, i):
    """reasons 0, 2, 4, 6 in turn"""
    return de.make_ballot(el, [de.nonzero(rng) for _ in range(el.n + 1)], [rng.randrange(R) for _ in range(el.n_rest)], rng, bump_psi=int(i % 4 in (1, 3)),
                          bump_z=int(i % 4 in (2, 3)))


SHAPES = {1: 0, 2: 3, 7: 0, 8: 3, 16: 0, 17: 3, 25: 0, 64: 3}       # msg_size: n_rest


@pytest.fixture(scope="module")
def elections(ctx, cref):
    made = {}

    def get(n):
        if n not in made:
            rng = de.rng(300 + n)
            el = de.Election(rng, n, SHAPES[n])
            b = de.ballot_batch(el, [ordinary_ballot(el, rng, i) for i in range(66)])
            assert set(b["want"]) == {0, 2, 4, 6} and b["want"][63:66] == [6, 0, 2]
            made[n] = (make_verifier(ctx, el), b)
        return made[n]
    yield get
    for ver, _ in made.values():
        ver.free()


@pytest.mark.parametrize("group", ["default", "one", "all", "above"])
@pytest.mark.parametrize("n", list(SHAPES))
def test_saver_shapes_and_groupings(ctx, elections, n, group):
    """n + 2 = 3, 4, 9, 10, 18, 19, 27, 66 pairs against groups of 9 (one group, exact multiples, one more than a multiple, 8 groups), of
    1, of n + 2 and of more than n + 2 (clamped)"""
    ver, b = elections(n)
    value = dict(default=None, one=1, all=n + 2, above=n + 7)[group]
    assert with_option(ctx, "saver_verify_group", value, 9, lambda: saver_reasons(ctx, ver, b)) == b["want"]


def test_saver_largest_key(ctx, cref):
    """msg_size 1022: 1026 prepared arguments, 115 groups of the ciphertext equation"""
    rng = de.rng(399)
    el = de.Election(rng, 1022, 3)
    b = de.ballot_batch(el, [ordinary_ballot(el, rng, i) for i in range(3)])
    assert b["want"] == [0, 2, 4]
    ver = make_verifier(ctx, el)
    try:
        assert saver_reasons(ctx, ver, b) == b["want"]
    finally:
        ver.free()


def saver_batch(ctx, seed, n_rest, fixed, cases):
    """msg_size 4.  cases: (us, xs, the branches the accumulation must take, make_ballot keywords), xs a function of (rng, election) and us of
    (rng, election, xs);
    each becomes an accepted member, one failing equation 1 alone and one failing equation 2 alone"""
    rng = de.rng(seed)
    el = de.Election(rng, 4, n_rest, fixed(rng) if fixed else None)
    specials = []
    for us, xs, branches, kw in cases:
        xs = xs(rng, el)
        us = us(rng, el, xs)
        us = [u % R for u in us]
        ev, acc = walk(list(zip(el.key.g[5:], xs)) if n_rest else [], [el.key.g[0]] + us)
        assert branches <= ev, (branches, ev)
        assert (acc or 0) == el.acc(us, xs)
        for bump_psi, bump_z in ((0, 0), (1, 0), (0, 1)):
            m = de.make_ballot(el, us, xs, rng, bump_psi=bump_psi, bump_z=bump_z, **kw)
            assert de.ballot_reason(el, m["us"], m["psi"], m["xs"], m["s"], m["t"], m["z"]) == 2 * bump_psi + 4 * bump_z
            specials.append(m)
    b = de.ballot_batch(el, place(specials, 66, lambda i: ordinary_ballot(el, rng, i)))
    ver = make_verifier(ctx, el)
    try:
        got = {chunk: with_option(ctx, "pairing_chunk", chunk, 1 << 14, lambda: saver_reasons(ctx, ver, b)) for chunk in (None, 20)}
    finally:
        ver.free()
    assert got[None] == b["want"]
    assert got[20] == b["want"]


def rnd_us(rng, el, xs):
    return [de.nonzero(rng) for _ in range(el.n + 1)]


def rnd_xs(rng, el):
    return [rng.randrange(R) for _ in range(el.n_rest)]


def ciphertext_cases(xs):
    """exceptional ciphertexts beside the rest inputs xs(rng, election); the additions of c_0 .. c_n follow that of G_0, which follows
    the scalar part"""
    def change(fn):
        def us(rng, el, xs):
            u = rnd_us(rng, el, xs); fn(u, el, xs); return u
        return us

    def equal(u, el, xs): u[2] = u[1]
    def opposite(u, el, xs): u[2] = R - u[1]
    def one_zero(u, el, xs): u[3] = 0
    def all_zero(u, el, xs): u[:] = [0] * 5
    def u0_is_g0(u, el, xs): u[0] = el.key.g[0]
    def u0_is_minus_g0(u, el, xs): u[0] = R - el.key.g[0]
    def total_zero(u, el, xs): u[4] = 0; u[4] = (-el.acc(u, xs)) % R
    return [(rnd_us, xs, set(), {}),
            (change(equal), xs, set(), {}),
            (change(opposite), xs, set(), {}),
            (change(one_zero), xs, set(), {}),
            (change(all_zero), xs, set(), {}),
            (change(u0_is_g0), xs, {"equal, affine accumulator"}, {}),
            (change(u0_is_minus_g0), xs, {"opposite", "left infinity again"}, {}),
            (change(total_zero), xs, {"opposite"}, {}),
            (rnd_us, xs, set(), dict(s=0)),
            (rnd_us, xs, set(), dict(t=0)),
            (rnd_us, xs, set(), dict(z=0))]


def test_saver_exceptional_ballots_without_rest_inputs(ctx, cref):
    """u_1 = u_2, u_1 = -u_2, a zero u_j, all of them and psi zero, u_0 = g_0 (the accumulator doubles at its first ciphertext addition:
    the scalar part is empty), u_0 = -g_0, the whole sum infinity, A, B or C at infinity"""
    cases = ciphertext_cases(lambda rng, el: [])
    saver_batch(ctx, 401, 0, None, cases)


def test_saver_exceptional_ballots_with_zero_and_edge_rest_inputs(ctx, cref):
    """the same with three rest inputs, all zero (u_0 = g_0 still meets the affine G_0), then rest scalars of r - 1 and 0 among random ones"""
    zero = lambda rng, el: [0, 0, 0]
    edge = lambda rng, el: [R - 1, 0, rng.randrange(R)]
    cases = ciphertext_cases(zero) + [(rnd_us, edge, set(), {}), (rnd_us, lambda rng, el: [0, R - 1, R - 1], set(), {})]
    saver_batch(ctx, 402, 3, None, cases)


def test_saver_exceptional_window_loop(ctx, cref):
    """equal and opposite points inside the 4-bit window loop over the key's table, which ciphertext members never reach: g_6 = g_5 with
    x_1 = x_2 (affine accumulator), g_6 = 16 g_5 with digits one window apart (ZZ != 1), g_6 = -g_5 (infinity doubled on, and left
    again through x_3 or through G_0)"""
    def keys(mult):
        def fixed(rng):
            g5 = de.nonzero(rng)
            return {5: g5, 6: mult * g5 % R}
        return fixed
    full = lambda rng: rng.randrange(R // 2, R)
    saver_batch(ctx, 403, 3, keys(1), [(rnd_us, lambda rng, el: [x := full(rng), x, rng.randrange(R)], {"equal, affine accumulator"}, {})])
    later = lambda w: (rnd_us, lambda rng, el: [0x10 << (4 * w), 1 << (4 * w), rng.randrange(16 ** (w + 1))], {"equal, ZZ != 1"}, {})
    saver_batch(ctx, 404, 3, keys(16), [later(0), later(31), later(62)])
    saver_batch(ctx, 405, 3, keys(R - 1), [(rnd_us, lambda rng, el: [x := full(rng), x, 0], {"opposite", "infinity doubled", "left infinity again"}, {}),
                                           (rnd_us, lambda rng, el: [x := full(rng), x, full(rng)], {"opposite", "left infinity again"}, {})])
