"""GPU: the witness check -- vsp_r1cs_check_batch / vsp_r1cs_is_satisfied (bp.is_satisfied(), common.hpp:1109-1128) and option
"prove_check_witness" of every prover entry point.  Every expectation comes from Python integers over the exported CSR matrices or from the
oracle (cref.R1CS.is_satisfied, cref.Keypair.prove, oracle/pairing.py), never from the library."""
import ctypes as C
import random

import numpy as np
import pytest

import bls12_381 as o
from conftest import I, L, fr_array, fr_ints

import vote_saver_protocol_amd as v

pytestmark = pytest.mark.gpu

R = o.R
OK, ERR_ARG, ERR_UNSATISFIED = 0, -1, -5


# ---- the reference: Python integers over CSR triples (row_ptr, col, coefficient ints)
def csr_ints(mats):
    return [(np.asarray(rp).astype(np.int64).tolist(), np.asarray(ci).astype(np.int64).tolist(), fr_ints(co) if len(ci) else []) for rp, ci, co in mats]


def failing_rows(mats, nc, z):
    """rows i < nc with (A z)[i] (B z)[i] != (C z)[i] mod r; z = [1, witness...] as ints"""
    def row(m, i):
        rp, ci, co = m
        return sum(co[e] * z[ci[e]] for e in range(rp[i], rp[i + 1])) % R
    return [i for i in range(nc) if row(mats[0], i) * row(mats[1], i) % R != row(mats[2], i)]


def expect(mats, nc, z):
    """(status bit 1, first_bad_row, bad_rows) of a canonical assignment"""
    f = failing_rows(mats, nc, z)
    return (2 if f else 0), (f[0] if f else nc), len(f)


def z_of(wit):
    return [1] + fr_ints(wit)


def wit_of(z):
    return fr_array(z[1:])


def run_check(ctx, dcs, wits):
    status, first, bad = dcs.check(ctx, np.stack(wits))
    return status.tolist(), first.tolist(), bad.tolist()


class Synth:
    """a synthetic system (row j defines variable ni + 1 + j: a boolean row z_k z_k = z_k or a product row z_a z_b = z_k), uploaded as the
    prover tests upload theirs"""

    def __init__(self, ctx, cref, nc, ni, seed):
        self.nc, self.ni = nc, ni
        self.cs, self.wit = cref.R1CS.synth(nc, ni, seed)
        self.exported = self.cs.export()
        self.dcs = v.R1CS(ctx, nc, ni, self.cs.num_vars, *self.exported)
        self.mats = csr_ints(self.exported)
        self.cols = [m[1] for m in self.mats]                     # one term per row: the column of row j in A, B, C

    def break_row(self, z, j, value=None):
        """z with the wire row j defines changed so that row j fails (a boolean wire -> 2, a product wire -> a b + 1, or `value`), and every
        later product row recomputed, so that row j is the ONLY failing row"""
        z = list(z)
        a, b, k = (c[j] for c in self.cols)
        assert k == self.ni + 1 + j
        z[k] = value if value is not None else (2 if a == b == k else (z[a] * z[b] + 1) % R)
        return self.repair(z, j + 1)

    def repair(self, z, first_row=0):
        """every product row from first_row on recomputed from the wires it reads"""
        z = list(z)
        for j in range(first_row, self.nc):
            a, b, k = (c[j] for c in self.cols)
            if not a == b == k:
                z[k] = z[a] * z[b] % R
        return z

    def product_rows(self):
        return [j for j in range(self.nc) if not self.cols[0][j] == self.cols[1][j] == self.cols[2][j]]


# make_evaluation_domain(num_constraints + num_inputs + 1): 304 -> step domain 256 + 64 = 320, rows no multiple of 64 or 256 | 706 -> step
# domain 512 + 256 | 66 -> step domain 64 + 2, exactly one wave of rows | 512 -> the basic domain, m = 512, rows no multiple of 64
SIZES = [(300, 3), (700, 5), (64, 1), (508, 3)]
DOMAINS = {(300, 3): (320, True), (700, 5): (768, True), (64, 1): (66, True), (508, 3): (512, False)}


@pytest.fixture(scope="module")
def systems(ctx, cref):
    d = {(nc, ni): Synth(ctx, cref, nc, ni, seed=1000 + nc) for nc, ni in SIZES}
    for size, s in d.items():
        assert (s.cs.m, s.cs.is_step) == DOMAINS[size] and s.dcs.m == s.cs.m
    yield d
    for s in d.values():
        s.dcs.free(); s.cs.free()


# ---- 1. synthetic systems
@pytest.mark.parametrize("size", SIZES)
def test_satisfying_witnesses_are_accepted(ctx, systems, size):
    s = systems[size]
    wits = [s.wit] + [s.cs.resample_witness(seed) for seed in (1, 2, 3)] + [s.cs.resample_witness(0, zero=True)]
    for w in wits:
        assert s.cs.is_satisfied(w) and expect(s.mats, s.nc, z_of(w)) == (0, s.nc, 0)
        assert s.dcs.is_satisfied(ctx, w) is True
    status, first, bad = run_check(ctx, s.dcs, wits)
    assert status == [0] * 5 and first == [s.nc] * 5 and bad == [0] * 5


@pytest.mark.parametrize("size", SIZES)
def test_one_failing_row_is_found_at_its_index(ctx, systems, size):
    s = systems[size]
    rows = [j for j in (0, 63, 64, 255, 256, s.nc - 1) if j < s.nc]
    rows = sorted(set(rows))
    wits = []
    for j in rows:
        z = s.break_row(z_of(s.wit), j)
        assert failing_rows(s.mats, s.nc, z) == [j]
        wits.append(wit_of(z))
        assert not s.cs.is_satisfied(wits[-1]) and s.dcs.is_satisfied(ctx, wits[-1]) is False
    status, first, bad = run_check(ctx, s.dcs, wits)
    assert status == [2] * len(rows) and first == rows and bad == [1] * len(rows)
    # vsp_r1cs_is_satisfied reports the row too
    ok, row = C.c_int(7), C.c_uint64(0)
    w = np.ascontiguousarray(wits[-1])
    assert ctx.lib.vsp_r1cs_is_satisfied(ctx.h, s.dcs.h, w.ctypes.data_as(C.c_void_p), C.byref(ok), C.byref(row)) == OK
    assert ok.value == 0 and row.value == rows[-1]


@pytest.mark.parametrize("size", SIZES)
def test_several_failing_rows_minimum_and_exact_count(ctx, systems, size):
    s = systems[size]
    rng = random.Random(size[0])
    wits, want = [], []
    for trial in range(6):
        z = z_of(s.wit)
        for k in rng.sample(range(1, len(z)), min(2 + 9 * trial, len(z) - 1)):      # wires changed without repair: their own rows and the rows that read them
            z[k] = rng.randrange(R)
        wits.append(wit_of(z)); want.append(expect(s.mats, s.nc, z))
    assert all(w[2] >= 2 for w in want)
    # the LAST rows only, then every row
    z = z_of(s.wit)
    z = s.break_row(s.break_row(z, s.nc - 2), s.nc - 1)
    wits.append(wit_of(z)); want.append(expect(s.mats, s.nc, z)); assert want[-1] == (2, s.nc - 2, 2)
    z = [1] + [5] * (len(z) - 1)
    wits.append(wit_of(z)); want.append(expect(s.mats, s.nc, z)); assert want[-1] == (2, 0, s.nc)      # 25 != 5 on every row
    status, first, bad = run_check(ctx, s.dcs, wits)
    assert list(zip(status, first, bad)) == want


@pytest.mark.parametrize("size", [(300, 3), (700, 5)])
def test_products_that_wrap_around_r(ctx, systems, size):
    """operands r - 1, r - 2: the product is far beyond 2^256 before the reduction.  c = a b mod r holds, c = a b + 1 mod r does not"""
    s = systems[size]
    wits, want, probe = [], [], []
    for j in s.product_rows()[:4]:
        a, b, k = (c[j] for c in s.cols)
        for delta in (0, 1):
            z = z_of(s.wit)
            z[a] = R - 1; z[b] = R - 2 if b != a else R - 1
            z[k] = (z[a] * z[b] + delta) % R
            f = failing_rows(s.mats, s.nc, z)
            assert (j in f) == bool(delta)
            wits.append(wit_of(z)); want.append(expect(s.mats, s.nc, z)); probe.append((j, delta))
    status, first, bad = run_check(ctx, s.dcs, wits)
    assert list(zip(status, first, bad)) == want
    # the pairs differ by exactly row j
    for t in range(0, len(want), 2):
        assert want[t + 1][2] == want[t][2] + 1
    # and with the rest of the witness consistent: inputs near r, every product row recomputed, then one row off by one
    z = z_of(s.wit)
    for k in range(1, s.ni + 1):
        z[k] = R - k
    z = s.repair(z)
    assert max(z[1:]) > R - 10 and failing_rows(s.mats, s.nc, z) == []
    j = s.product_rows()[-1]
    zb = s.break_row(z, j)
    assert failing_rows(s.mats, s.nc, zb) == [j]
    status, first, bad = run_check(ctx, s.dcs, [wit_of(z), wit_of(zb)])
    assert (status, first, bad) == ([0, 2], [s.nc, j], [0, 1])


# ---- 2. a hand-built system with multi-term rows
HAND_NC, HAND_NV = 12, 8
HAND_ALWAYS = {3, 4, 6, 9, 11}              # rows that hold for every assignment (0 = 0, 1 = 1, an identity)


def hand_built():
    """8 variables (columns 0..8, column 0 the constant), 12 rows; terms (column, coefficient) per row of A, B, C.  Rows 10, 0, 1, 2, 5, 7, 8
    each define one wire (z2, z3, z4, z5, z6, z7, z8), so each can be made to fail alone; z1 is free"""
    rows = [
        ([(1, 1)], [(2, 1)], [(3, 1)]),                                       # 0  z1 z2 = z3
        ([(1, 2), (2, 3), (0, 5)], [(0, 1)], [(4, 1)]),                       # 1  (2 z1 + 3 z2 + 5) 1 = z4          the constant column
        ([(1, 1), (1, 1), (1, R - 1)], [(2, 1), (3, 4)], [(5, 1)]),           # 2  (z1 + z1 - z1)(z2 + 4 z3) = z5    repeated columns, r - 1
        ([], [], []),                                                         # 3  0 0 = 0                           all empty
        ([], [(6, 1)], []),                                                   # 4  0 z6 = 0                          empty A and C
        ([(6, 1)], [(6, 1)], []),                                             # 5  z6 z6 = 0                         empty C: holds only for z6 = 0
        ([(3, R - 1), (4, 1)], [(0, R - 1)], [(3, 1), (4, R - 1)]),           # 6  (z4 - z3)(-1) = z3 - z4           an identity through r - 1
        ([(7, 1)], [(7, 1), (0, R - 1)], []),                                 # 7  z7 (z7 - 1) = 0                   boolean, empty C
        ([(5, 1), (7, 3)], [(1, 1), (2, 1)], [(8, 1), (8, 1), (8, R - 1), (0, 0)]),   # 8  (z5 + 3 z7)(z1 + z2) = z8   a zero coefficient
        ([(0, 1)], [(0, 1)], [(0, 1)]),                                       # 9  1 1 = 1
        ([(2, R - 1)], [(2, R - 1)], [(2, 1), (2, 1), (2, R - 1)]),           # 10 z2^2 = z2
        ([(4, 7), (3, 1)], [], []),                                           # 11 (7 z4 + z3) 0 = 0                 empty B and C
    ]
    mats = []
    for which in range(3):
        rp, ci, co = [0], [], []
        for r in rows:
            for col, coef in r[which]:
                ci.append(col); co.append(coef)
            rp.append(len(ci))
        mats.append((np.array(rp, np.uint32), np.array(ci, np.uint32), fr_array(co)))
    return mats


def hand_assign(z1, z2=1, z6=0, z7=1, force=None):
    """[1, z1 .. z8]: the wires the rows define computed in order, except the ones `force` sets -- a forced wire breaks its own row only"""
    force = force or {}
    z = [1, z1 % R, z2, 0, 0, 0, z6, z7, 0]
    z[3] = force.get(3, z[1] * z[2] % R)
    z[4] = force.get(4, (2 * z[1] + 3 * z[2] + 5) % R)
    z[5] = force.get(5, z[1] * (z[2] + 4 * z[3]) % R)
    z[8] = force.get(8, (z[5] + 3 * z[7]) * (z[1] + z[2]) % R)
    return z


def hand_cases():
    """[(assignment, rows expected to fail or None = whatever the reference computes)]"""
    cases = []
    for z1 in (1, 12345, R - 1, R - 3, (R + 1) // 2):
        for z2 in (0, 1):
            for z7 in (0, 1):
                cases.append((hand_assign(z1, z2=z2, z7=z7), []))
    for z1 in (7, R - 1):
        ok = hand_assign(z1)
        cases.append((hand_assign(z1, force={3: (ok[3] + 1) % R}), [0]))
        cases.append((hand_assign(z1, force={4: (ok[4] + 1) % R}), [1]))
        cases.append((hand_assign(z1, force={5: (ok[5] + 1) % R}), [2]))
        cases.append((hand_assign(z1, z6=9), [5]))                       # z6 z6 = 0 fails while 0 z6 = 0 (row 4) holds
        cases.append((hand_assign(z1, z6=R - 1), [5]))
        cases.append((hand_assign(z1, z7=2), [7]))
        cases.append((hand_assign(z1, force={8: (ok[8] + 1) % R}), [8]))
        cases.append((hand_assign(z1, z2=2), [10]))
        cases.append((hand_assign(z1, z2=R - 1), [10]))
        cases.append((hand_assign(z1, z2=2, z6=1, z7=3, force={3: 0, 8: 1}), None))
        for k in range(1, HAND_NV + 1):                                   # every wire in turn off by one and at r - 1, nothing repaired
            for val in (None, R - 1):
                z = list(ok); z[k] = (z[k] + 1) % R if val is None else val
                cases.append((z, None))
    return cases


def test_hand_built_system_row_by_row(ctx):
    exported = hand_built()
    mats = csr_ints(exported)
    dcs = v.R1CS(ctx, HAND_NC, 2, HAND_NV, *exported)
    cases = hand_cases()
    alone = set()
    for z, rows in cases:
        f = failing_rows(mats, HAND_NC, z)
        assert rows is None or f == rows, (z, rows, f)
        assert not HAND_ALWAYS & set(f)
        if len(f) == 1:
            alone.add(f[0])
    assert alone == set(range(HAND_NC)) - HAND_ALWAYS                       # every row that can fail was seen failing alone
    want = [expect(mats, HAND_NC, z) for z, _ in cases]
    assert any(w[2] >= 3 for w in want)
    status, first, bad = run_check(ctx, dcs, [wit_of(z) for z, _ in cases])
    assert list(zip(status, first, bad)) == want
    dcs.free()


# ---- 3. batches
def mixed_batch(s, K, bad_members):
    """K witnesses: distinct satisfying assignments, the members in bad_members broken at a row of their own"""
    wits, want = [], []
    base = [s.wit] + [s.cs.resample_witness(100 + t) for t in range(4)]
    for k in range(K):
        z = z_of(base[k % len(base)])
        if k in bad_members:
            z = s.break_row(z, (37 * k + 5) % s.nc)
            if k % 3 == 0:
                z = s.break_row(z, s.nc - 1)
        wits.append(wit_of(z)); want.append(expect(s.mats, s.nc, z))
    return wits, want


@pytest.mark.parametrize("K,bad_members", [(5, {0, 4}), (5, {2}), (64, {0, 1, 31, 32, 63}), (65, {0, 63, 64}), (130, {0, 63, 64, 65, 127, 128, 129})])
def test_batches_with_good_and_bad_members(ctx, systems, K, bad_members):
    s = systems[(300, 3)]
    wits, want = mixed_batch(s, K, bad_members)
    assert [w[0] for w in want] == [2 if k in bad_members else 0 for k in range(K)]
    got = run_check(ctx, s.dcs, wits)
    assert list(zip(*got)) == want
    # the verdicts do not depend on the split: one call per member
    for k in sorted(bad_members | {1, K - 2}):
        one = run_check(ctx, s.dcs, [wits[k]])
        assert (one[0][0], one[1][0], one[2][0]) == want[k]


def test_step_domain_batch_crossing_the_piece_boundary(ctx, systems):
    s = systems[(700, 5)]
    wits, want = mixed_batch(s, 66, {0, 5, 63, 64, 65})
    assert list(zip(*run_check(ctx, s.dcs, wits))) == want


# ---- 4. values that are not canonical
@pytest.mark.parametrize("size", [(300, 3), (64, 1)])
def test_a_value_not_below_r_is_flagged(ctx, systems, size):
    s = systems[size]
    used = set(s.cols[0]) | set(s.cols[1])
    read_later = [k for k in range(1, s.ni + 1) if k in used]              # an input that some constraint reads
    unread = [k for k in range(1, s.ni + 1) if k not in used]              # ... and one that none reads, if the system has one
    in_c = s.ni + 1 + s.nc // 2                                            # a wire its own row defines
    wits, want_bit0 = [], []
    for value in (R, (1 << 256) - 1):
        for k in [in_c] + read_later[:1] + unread[:1] + [len(s.wit)]:      # the last wire too
            w = s.wit.copy(); w[k - 1] = L(value, 4)
            wits += [s.wit, w]; want_bit0 += [0, 1]
    wits.append(s.cs.resample_witness(9)); want_bit0.append(0)
    status, first, bad = run_check(ctx, s.dcs, wits)
    assert [x & 1 for x in status] == want_bit0
    for k, flagged in enumerate(want_bit0):
        if not flagged:
            assert (status[k], first[k], bad[k]) == (0, s.nc, 0)           # the neighbours are unaffected
        else:
            assert first[k] <= s.nc and bad[k] <= s.nc
            assert s.dcs.is_satisfied(ctx, wits[k]) is False
    # r in a wire that NO constraint names: the rows all hold, only bit 0 tells
    exported = hand_built()
    dcs = v.R1CS(ctx, HAND_NC, 2, HAND_NV + 1, *exported)                  # a ninth variable no row reads
    z = hand_assign(R - 1) + [0]
    plain, with_r, with_max = wit_of(z), wit_of(z), wit_of(z)
    with_r[HAND_NV] = L(R, 4); with_max[HAND_NV] = L((1 << 256) - 1, 4)
    status, first, bad = run_check(ctx, dcs, [plain, with_r, plain, with_max])
    assert (status, first, bad) == ([0, 1, 0, 1], [12] * 4, [0] * 4)
    dcs.free()


# ---- 5 / 6. the prover
class Proving:
    def __init__(self, ctx, cref, s, seed):
        gen = o.splitmix64(seed)
        self.s = s
        tox = fr_array([o.rand_fr(gen) for _ in range(5)])
        self.kp = cref.Keypair(s.cs, tox)
        self.q = [ctx.upload_bases(self.kp.part(n), g) for n, g in (("A_query", 1), ("B_query_g1", 1), ("B_query_g2", 2), ("H_query", 1), ("L_query", 1))]
        self.pk = v.ProvingKey(ctx, self.kp.part("alpha_g1")[0], self.kp.part("beta_g1")[0], self.kp.part("beta_g2")[0], self.kp.part("delta_g1")[0],
                               self.kp.part("delta_g2")[0], *self.q)
        self.r = [L(o.rand_fr(gen), 4) for _ in range(8)]
        self.t = [L(o.rand_fr(gen), 4) for _ in range(8)]
        self.rnd = fr_array([o.rand_fr(gen) for _ in range(3 * 2 + 2)])
        self.r_enc = L(o.rand_fr(gen), 4)

    def oracle_bytes(self, wit, r, s_, **kw):
        A, B, Cc = self.kp.prove(wit, r, s_, **kw)
        return A, B, Cc, o.g1_compress(o.g1_from_limbs(A)) + o.g2_compress(o.g2_from_limbs(B)) + o.g1_compress(o.g1_from_limbs(Cc))

    def free(self):
        self.pk.free(); [x.free() for x in self.q]; self.kp.free()


@pytest.fixture(scope="module")
def proving(ctx, cref, systems):
    p = Proving(ctx, cref, systems[(300, 3)], seed=4242)
    yield p
    p.free()


@pytest.fixture
def checking(ctx):
    """option prove_check_witness = 1 for one test on the shared context"""
    ctx.set_option("prove_check_witness", 1)
    yield ctx
    ctx.set_option("prove_check_witness", 0)


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def raw_prove(ctx, p, wit, r, s_):
    """vsp_groth16_prove through ctypes, outputs preset to a pattern: -> (rc, A, B, C, proof bytes)"""
    wit = np.ascontiguousarray(wit)
    A = np.full(12, 0xA5A5, np.uint64); B = np.full(24, 0xA5A5, np.uint64); Cc = np.full(12, 0xA5A5, np.uint64); proof = np.full(192, 0x5A, np.uint8)
    rc = ctx.lib.vsp_groth16_prove(ctx.h, p.s.dcs.h, p.pk.h, _p(wit), _p(r), _p(s_), None, None, _p(A), _p(B), _p(Cc), _p(proof))
    return rc, A, B, Cc, proof.tobytes()


def bad_witness(s, row, base=None):
    z = s.break_row(z_of(s.wit if base is None else base), row)
    assert failing_rows(s.mats, s.nc, z) == [row]
    return wit_of(z)


def test_prover_without_the_option_proves_a_bad_witness_as_before(ctx, proving):
    p = proving
    bad = bad_witness(p.s, 123)
    assert ctx.lib.vsp_set_option(ctx.h, b"prove_check_witness", 0) == OK
    rc, A, B, Cc, proof = raw_prove(ctx, p, bad, p.r[0], p.t[0])
    eA, eB, eC, ebytes = p.oracle_bytes(bad, p.r[0], p.t[0])
    assert rc == OK and np.array_equal(A, eA) and np.array_equal(B, eB) and np.array_equal(Cc, eC) and proof == ebytes
    # and the batch: member 1 bad, all three as the oracle's prover computes them
    wits = np.stack([p.s.wit, bad, p.s.cs.resample_witness(5)])
    out = v.groth16_prove_batch(ctx, p.s.dcs, p.pk, wits, np.stack(p.r[:3]), np.stack(p.t[:3]))
    for k in range(3):
        assert out[3][k] == p.oracle_bytes(wits[k], p.r[k], p.t[k])[3]


def test_single_proof_refuses_an_unsatisfying_witness(checking, proving, cref):
    ctx, p = checking, proving
    good = p.s.cs.resample_witness(77)
    want_good = p.oracle_bytes(good, p.r[1], p.t[1])
    for row in (0, 64, 299):
        bad = bad_witness(p.s, row)
        # plain
        rc, A, B, Cc, proof = raw_prove(ctx, p, bad, p.r[0], p.t[0])
        assert rc == ERR_UNSATISFIED and not A.any() and not B.any() and not Cc.any() and proof == bytes(192)
        assert ctx.stat("prove_first_bad_row") == row and f"constraint {row} " in ctx.last_error()
        with pytest.raises(v.Unsatisfied) as e:
            v.groth16_prove(ctx, p.s.dcs, p.pk, bad, p.r[0], p.t[0])
        assert e.value.first_bad_row == row and isinstance(e.value, v.VspError)
        # packed, in two halves: the verdict survives from the launch to the finish
        v.groth16_prove_launch(ctx, p.s.dcs, p.pk, v.PackedWitness(bad), p.r[0], p.t[0])
        A = np.full(12, 7, np.uint64); B = np.full(24, 7, np.uint64); Cc = np.full(12, 7, np.uint64); proof = np.full(192, 7, np.uint8)
        assert ctx.lib.vsp_groth16_prove_finish(ctx.h, _p(A), _p(B), _p(Cc), _p(proof)) == ERR_UNSATISFIED
        assert not A.any() and not B.any() and not Cc.any() and not proof.any() and ctx.stat("prove_first_bad_row") == row
        # the context proves a good witness right afterwards, plain and packed
        got = v.groth16_prove(ctx, p.s.dcs, p.pk, good, p.r[1], p.t[1])
        assert got[3] == want_good[3] and np.array_equal(got[0], want_good[0]) and ctx.stat("prove_first_bad_row") == p.s.nc
        v.groth16_prove_launch(ctx, p.s.dcs, p.pk, v.PackedWitness(good), p.r[1], p.t[1])
        assert v.groth16_prove_finish(ctx)[3] == want_good[3]
    # a value >= r keeps its own error
    w = good.copy(); w[200] = L(R, 4)
    rc, *_ = raw_prove(ctx, p, w, p.r[0], p.t[0])
    assert rc == ERR_ARG and "canonical" in ctx.last_error()
    assert v.groth16_prove(ctx, p.s.dcs, p.pk, good, p.r[1], p.t[1])[3] == want_good[3]


def test_saver_encrypt_refuses_an_unsatisfying_witness(checking, proving, cref):
    ctx, p = checking, proving
    nmsg = 2
    gabc = p.kp.part("gamma_ABC_g1")
    pk_w, _, _ = v.saver_generate_keypair(ctx, p.rnd, gabc, p.kp.part("delta_g1")[0], p.kp.part("gamma_g1")[0], nmsg)
    pk_c, _, _ = cref.saver_keygen(nmsg, p.kp.part("delta_g1")[0], p.kp.part("gamma_g1")[0], gabc[:nmsg + 1], p.rnd)
    assert np.array_equal(pk_w, pk_c)
    spk = v.SaverPublicKey(ctx, pk_w, gabc[:nmsg + 1], nmsg)
    bad = np.ascontiguousarray(bad_witness(p.s, 255))               # the message inputs are untouched
    ct = np.full((nmsg + 2, 12), 3, np.uint64); A = np.full(12, 3, np.uint64); B = np.full(24, 3, np.uint64); Cc = np.full(12, 3, np.uint64)
    proof = np.full(192, 3, np.uint8)
    msg = np.ascontiguousarray(bad[:nmsg])
    rc = ctx.lib.vsp_saver_encrypt(ctx.h, spk.h, p.s.dcs.h, p.pk.h, _p(msg), _p(bad), _p(p.r_enc), _p(p.r[2]), _p(p.t[2]), _p(ct), _p(A), _p(B), _p(Cc), _p(proof))
    assert rc == ERR_UNSATISFIED and not ct.any() and not A.any() and not B.any() and not Cc.any() and not proof.any()
    assert ctx.stat("prove_first_bad_row") == 255
    with pytest.raises(v.Unsatisfied):
        v.saver_encrypt(ctx, spk, p.s.dcs, p.pk, bad[:nmsg], bad, p.r_enc, p.r[2], p.t[2])
    good = p.s.wit
    ct, (sa, sb, sc), blob = v.saver_encrypt(ctx, spk, p.s.dcs, p.pk, good[:nmsg], good, p.r_enc, p.r[2], p.t[2])
    want = p.oracle_bytes(good, p.r[2], p.t[2], P1=pk_c[-12:], r_enc=p.r_enc)
    assert blob == want[3] and np.array_equal(ct, cref.saver_encrypt_ct(nmsg, pk_c, gabc[:nmsg + 1], good[:nmsg], p.r_enc))
    spk.free()


def test_batch_of_eight_with_three_bad_members(ctx, proving):
    import pairing as pg
    p = proving
    K, bad_members = 8, {0: 17, 3: 256, 7: 299}
    wits = [p.s.cs.resample_witness(300 + k) for k in range(K)]
    for k, row in bad_members.items():
        wits[k] = bad_witness(p.s, row, base=wits[k])
    wits = np.stack(wits); r = np.stack(p.r[:K]); t = np.stack(p.t[:K])
    ctx.set_option("prove_check_witness", 0)
    off = v.groth16_prove_batch(ctx, p.s.dcs, p.pk, wits, r, t)
    singles = [v.groth16_prove(ctx, p.s.dcs, p.pk, wits[k], r[k], t[k]) for k in range(K) if k not in bad_members]
    ctx.set_option("prove_check_witness", 1)
    try:
        A = np.full((K, 12), 9, np.uint64); B = np.full((K, 24), 9, np.uint64); Cc = np.full((K, 12), 9, np.uint64); proofs = np.full((K, 192), 9, np.uint8)
        rc = ctx.lib.vsp_groth16_prove_batch(ctx.h, p.s.dcs.h, p.pk.h, _p(wits), K, _p(r), _p(t), _p(A), _p(B), _p(Cc), _p(proofs))
        assert rc == ERR_UNSATISFIED
        status = np.full(K, 0xEE, np.uint8); first = np.full(K, 0xEE, np.uint64)
        assert ctx.lib.vsp_groth16_prove_batch_verdicts(ctx.h, _p(status), _p(first)) == OK
        assert status.tolist() == [2 if k in bad_members else 0 for k in range(K)]
        assert first.tolist() == [bad_members.get(k, p.s.nc) for k in range(K)]
        assert ctx.lib.vsp_groth16_prove_batch_verdicts(ctx.h, _p(status), None) == OK
        good = [k for k in range(K) if k not in bad_members]
        for n, k in enumerate(good):
            assert np.array_equal(A[k], off[0][k]) and np.array_equal(B[k], off[1][k]) and np.array_equal(Cc[k], off[2][k]) and proofs[k].tobytes() == off[3][k]
            assert proofs[k].tobytes() == singles[n][3] and np.array_equal(A[k], singles[n][0])
        for k in bad_members:
            assert not A[k].any() and not B[k].any() and not Cc[k].any() and not proofs[k].any()
            assert any(off[0][k])                                    # without the option the member had (worthless) outputs
        k = good[2]
        vk = dict(alpha_g1=o.g1_from_limbs(p.kp.part("alpha_g1")[0]), beta_g2=o.g2_from_limbs(p.kp.part("beta_g2")[0]),
                  gamma_g2=o.g2_from_limbs(p.kp.part("gamma_g2")[0]), delta_g2=o.g2_from_limbs(p.kp.part("delta_g2")[0]),
                  gamma_ABC_g1=[o.g1_from_limbs(x) for x in p.kp.part("gamma_ABC_g1")])
        assert pg.groth16_verify(vk, [I(wits[k][i]) for i in range(p.s.ni)], (o.g1_from_limbs(A[k]), o.g2_from_limbs(B[k]), o.g1_from_limbs(Cc[k])))
        # the Python wrapper: the exception carries the verdicts and the outputs
        with pytest.raises(v.Unsatisfied) as e:
            v.groth16_prove_batch(ctx, p.s.dcs, p.pk, wits, r, t)
        assert e.value.status.tolist() == status.tolist() and e.value.first_bad_row.tolist() == first.tolist()
        assert e.value.results[3][good[0]] == off[3][good[0]] and e.value.results[3][0] == bytes(192)
        # an all-good batch with the option on is the batch with the option off
        allgood = np.stack([wits[k] for k in good])
        on = v.groth16_prove_batch(ctx, p.s.dcs, p.pk, allgood, r[:5], t[:5])
        st, fb = v.groth16_prove_batch_verdicts(ctx)
        assert st.tolist() == [0] * 5 and fb.tolist() == [p.s.nc] * 5
        ctx.set_option("prove_check_witness", 0)
        off5 = v.groth16_prove_batch(ctx, p.s.dcs, p.pk, allgood, r[:5], t[:5])
        assert on[3] == off5[3] and all(np.array_equal(a, b) for a, b in zip(on[:3], off5[:3]))
    finally:
        ctx.set_option("prove_check_witness", 0)


def test_batch_verdicts_survive_from_launch_to_finish(cref, systems):
    with v.Context(0) as c:
        status = np.zeros(8, np.uint8)
        assert c.lib.vsp_groth16_prove_batch_verdicts(c.h, _p(status), None) == ERR_ARG            # before any batch
        s = Synth(c, cref, 64, 1, seed=1064)
        p = Proving(c, cref, s, seed=99)
        wits = np.stack([s.wit, bad_witness(s, 63), s.cs.resample_witness(2), bad_witness(s, 0)])
        c.set_option("prove_check_witness", 1)
        v.groth16_prove_batch_launch(c, s.dcs, p.pk, wits, np.stack(p.r[:4]), np.stack(p.t[:4]))
        assert c.lib.vsp_groth16_prove_batch_verdicts(c.h, _p(status), None) == ERR_ARG            # launched, not finished
        # the stand-alone check refuses a context whose workspace a batch in flight owns
        st1 = np.zeros(1, np.uint8)
        assert c.lib.vsp_r1cs_check_batch(c.h, s.dcs.h, _p(np.ascontiguousarray(s.wit)), 1, _p(st1), None, None) == ERR_ARG
        with pytest.raises(v.Unsatisfied) as e:
            v.groth16_prove_batch_finish(c)
        assert e.value.status.tolist() == [0, 2, 0, 2] and e.value.first_bad_row.tolist() == [64, 63, 64, 0]
        for k in (0, 2):
            assert e.value.results[3][k] == p.oracle_bytes(wits[k], p.r[k], p.t[k])[3]
        st, fb = v.groth16_prove_batch_verdicts(c, 4)
        assert st.tolist() == [0, 2, 0, 2] and fb.tolist() == [64, 63, 64, 0]
        # a batch without the option leaves no verdicts behind
        c.set_option("prove_check_witness", 0)
        v.groth16_prove_batch(c, s.dcs, p.pk, wits[:1], np.stack(p.r[:1]), np.stack(p.t[:1]))
        assert c.lib.vsp_groth16_prove_batch_verdicts(c.h, _p(status), None) == ERR_ARG
        p.free(); s.dcs.free(); s.cs.free()


# ---- 7. arguments
def test_arguments(ctx, systems):
    s = systems[(64, 1)]
    w = np.ascontiguousarray(np.stack([s.wit, s.wit]))
    st = np.zeros(2, np.uint8); fb = np.zeros(2, np.uint64); br = np.zeros(2, np.uint64); ok = C.c_int(0)
    f = ctx.lib.vsp_r1cs_check_batch
    for count in (0, 2):
        assert f(None, s.dcs.h, _p(w), count, _p(st), _p(fb), _p(br)) == ERR_ARG
        assert f(ctx.h, None, _p(w), count, _p(st), _p(fb), _p(br)) == ERR_ARG
        assert f(ctx.h, s.dcs.h, None, count, _p(st), _p(fb), _p(br)) == ERR_ARG
        assert f(ctx.h, s.dcs.h, _p(w), count, None, _p(fb), _p(br)) == ERR_ARG
    assert f(ctx.h, s.dcs.h, _p(w), 0, _p(st), None, None) == OK
    assert f(ctx.h, s.dcs.h, _p(w), 2, _p(st), None, None) == OK and st.tolist() == [0, 0]
    assert f(ctx.h, s.dcs.h, _p(w), 2, _p(st), _p(fb), None) == OK and fb.tolist() == [64, 64]
    assert f(ctx.h, s.dcs.h, _p(w), 2, _p(st), None, _p(br)) == OK and br.tolist() == [0, 0]
    g = ctx.lib.vsp_r1cs_is_satisfied
    assert g(None, s.dcs.h, _p(w), C.byref(ok), None) == ERR_ARG
    assert g(ctx.h, None, _p(w), C.byref(ok), None) == ERR_ARG
    assert g(ctx.h, s.dcs.h, None, C.byref(ok), None) == ERR_ARG
    assert g(ctx.h, s.dcs.h, _p(w), None, None) == ERR_ARG
    assert g(ctx.h, s.dcs.h, _p(w), C.byref(ok), None) == OK and ok.value == 1
    assert ctx.lib.vsp_groth16_prove_batch_verdicts(None, _p(st), None) == ERR_ARG
    assert ctx.lib.vsp_groth16_prove_batch_verdicts(ctx.h, None, None) == ERR_ARG
    ctx.stats_reset()
    assert ctx.stat("r1cs_check_ms") == 0
    s.dcs.check(ctx, w)
    assert ctx.stat("r1cs_check_ms") > 0
    empty = s.dcs.check(ctx, np.zeros((0, s.cs.num_vars, 4), np.uint64))
    assert all(len(x) == 0 for x in empty)


def test_a_system_without_constraints_is_satisfied_by_anything_canonical(ctx):
    ni, nv = 3, 5
    none = (np.zeros(1, np.uint32), np.zeros(0, np.uint32), np.zeros((0, 4), np.uint64))
    dcs = v.R1CS(ctx, 0, ni, nv, none, none, none)
    rng = random.Random(5)
    wits = [fr_array([rng.randrange(R) for _ in range(nv)]) for _ in range(3)] + [fr_array([R - 1] * nv), fr_array([0] * nv)]
    w_r = fr_array([1, 2, 3, 4, 5]); w_r[4] = L(R, 4)
    status, first, bad = run_check(ctx, dcs, wits + [w_r])
    assert (status, first, bad) == ([0] * 5 + [1], [0] * 6, [0] * 6)
    assert dcs.is_satisfied(ctx, wits[0]) is True and dcs.is_satisfied(ctx, w_r) is False
    dcs.free()
