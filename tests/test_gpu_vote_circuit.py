"""GPU tests of the voting circuit (vsp_vote_circuit_*, vsp_vote_witness_batch, vsp_vote_cast_batch) at depth 3, eid_bits 8,
n 4 and depth 5, eid_bits 70 (eid | sk spans the segments at another offset, eid_packed stays one scalar, the eid block is no multiple
of 3 bits).  Two judges of satisfaction: vsp_r1cs_check_batch, word for word what the prover consumes, and the big-integer judge of
tests/vote_circuit_model.py over the exported CSR, which knows nothing of the layout.  The public inputs are held against the model's
values and against the library's own hash and registry; the GPU's witnesses against the header's host path, word for word."""
import ctypes as C
import random

import numpy as np
import pytest

import jubjub_model as jm
import vote_circuit_model as vm
import vote_saver_protocol_amd as v
from conftest import rand_fr_array

pytestmark = pytest.mark.gpu

G = 3
ERR_ARG, ERR_UNSUPPORTED = -1, -4
SHAPES = [(3, 8, 4), (5, 70, 4)]


def key_array(keys):
    return np.array([jm.words(k) for k in keys], np.uint64).reshape(-1, 4)


def eid_words(bits):
    return np.array(jm.message_words(bits), np.uint64)


def sn_messages(eid, sks):
    """the rows eid | sk as vsp_pedersen_hash_batch takes them"""
    return np.array([jm.message_words(list(eid) + jm.bits_of(sk, 255)) for sk in sks], np.uint64)


@pytest.fixture(scope="module")
def gens():
    return jm.generators(G)


@pytest.fixture(scope="module")
def table(gens):
    return jm.Table(gens)


@pytest.fixture(scope="module")
def ped(ctx, gens):
    h = v.Pedersen(ctx, np.array([jm.point_words(g) for g in gens], np.uint64))
    yield h
    h.free()


class Election:
    """a circuit, every leaf of the tree registered, an eid.  Voter 1's sn digest is below 2^255 - r (found with the model)"""

    def __init__(self, ctx, ped, table, depth, eid_bits, n, hash_leaves, seed):
        self.ctx, self.ped, self.depth, self.nbits, self.n, self.hash_leaves = ctx, ped, depth, eid_bits, n, hash_leaves
        rng = random.Random(seed)
        self.eid = [rng.getrandbits(1) for _ in range(eid_bits)]
        self.sks = [rng.getrandbits(255) for _ in range(1 << depth)]
        while vm.serial_number(table, self.eid, self.sks[1]) >= (1 << 255) - jm.R:
            self.sks[1] = rng.getrandbits(255)
        self.pks = v.pedersen_hash_batch(ctx, ped, key_array(self.sks), 255)
        self.reg = v.Registry.build(ctx, ped, self.pks, depth, hash_leaves=bool(hash_leaves))
        self.circ = v.VoteCircuit(ctx, ped, n, eid_bits, depth, hash_leaves=bool(hash_leaves))
        self._judge = None
        last = (1 << depth) - 1
        alt = sum(1 << l for l in range(0, depth, 2))
        self.indices = [0, last, alt, last ^ alt, 1]                # both parities at every level: alt and its complement

    @property
    def judge(self):
        if self._judge is None:
            self._judge = vm.Judge(*self.circ.csr())
        return self._judge

    def witnesses(self, indices, votes=None, sks=None):
        votes = [i % self.n for i in range(len(indices))] if votes is None else votes
        sks = [self.sks[x] for x in indices] if sks is None else sks
        return self.circ.witness_batch(self.reg, eid_words(self.eid), key_array(sks), indices, votes)

    def both_refuse(self, wit):
        status, first, bad = self.circ.cs.check(self.ctx, wit[None])
        rows = self.judge.failing_rows(vm.witness_ints(wit))
        assert (status[0] != 0) == bool(rows) and bad[0] == len(rows) and (not rows or rows[0] == first[0])
        return bool(rows)

    def block(self, name):
        return self.circ.blocks[name][0]

    def free(self):
        self.circ.free(); self.reg.free()


@pytest.fixture(scope="module", params=[(s, hl) for s in SHAPES for hl in (1, 0)], ids=lambda p: f"depth{p[0][0]}_eid{p[0][1]}_leaves{p[1]}")
def el(request, ctx, ped, table):
    (depth, eid_bits, n), hl = request.param
    e = Election(ctx, ped, table, depth, eid_bits, n, hl, 500 + depth + hl)
    yield e
    e.free()


@pytest.fixture(scope="module")
def el3(ctx, ped, table):
    e = Election(ctx, ped, table, 3, 8, 4, 1, 77)
    yield e
    e.free()


def test_witnesses_satisfy_the_system_by_both_judges(el):
    assert el.circ.num_inputs == el.n + 1 + 4 and el.circ.cs.num_constraints == el.circ.num_constraints
    for K in (1, 5, 67):
        indices = [el.indices[i % len(el.indices)] for i in range(K)]
        wit, status = el.witnesses(indices)
        assert not status.any()
        verdict, first, bad = el.circ.cs.check(el.ctx, wit)
        assert not verdict.any() and (first == el.circ.num_constraints).all() and not bad.any()
        for k in sorted({0, K - 1, K // 2, min(64, K - 1)}):        # the model's judge on members of either piece
            assert el.judge.satisfied(vm.witness_ints(wit[k])), (K, k)


def test_public_inputs_are_the_protocols(el, table):
    wit, status = el.witnesses(el.indices)
    assert not status.any()
    root = el.reg.root()
    sn_lib = v.digest_scalars(v.pedersen_hash_batch(el.ctx, el.ped, sn_messages(el.eid, [el.sks[x] for x in el.indices]), el.nbits + 255))
    rt_lib = el.reg.rt_scalars()
    ni = el.circ.num_inputs
    for k, x in enumerate(el.indices):
        vote = k % el.n
        assert vm.witness_ints(wit[k, :ni]) == vm.public_inputs(table, el.n, el.eid, el.sks[x], vote, vm.from_words(root))
        assert vm.witness_ints(wit[k, :el.n]) == [1 if i == vote else 0 for i in range(el.n)]
        assert np.array_equal(wit[k, el.block("SN_PACKED"):el.block("SN_PACKED") + 2], sn_lib[k])
        assert np.array_equal(wit[k, el.block("RT_PACKED"):el.block("RT_PACKED") + 2], rt_lib)
        assert el.circ.blocks["EID_PACKED"][1] == 1 and vm.from_words(wit[k, el.block("EID_PACKED")]) == sum(b << i for i, b in enumerate(el.eid))


def test_gpu_witnesses_equal_the_host_path_word_for_word(el):
    wit, status = el.witnesses(el.indices)
    paths = el.reg.paths(el.indices)
    leaves = el.reg.nodes(0)
    for k, x in enumerate(el.indices):
        host, leaf = el.circ.witness_host(eid_words(el.eid), jm.words(el.sks[x]), x, k % el.n, paths[k])
        assert np.array_equal(leaf, leaves[x])
        assert np.array_equal(wit[k], host), (k, x)


def test_forced_lane_groups_do_not_change_a_witness(ctx, ped, el3):
    want, _ = el3.witnesses(el3.indices)
    try:
        for lanes in (1, 16, 64):
            ctx.set_option("pedersen_lanes", lanes)
            reg = v.Registry.build(ctx, ped, el3.pks, el3.depth, hash_leaves=True)
            got, status = el3.circ.witness_batch(reg, eid_words(el3.eid), key_array([el3.sks[x] for x in el3.indices]), el3.indices, [i % el3.n for i in range(len(el3.indices))])
            reg.free()
            assert not status.any() and np.array_equal(got, want)
    finally:
        ctx.set_option("pedersen_lanes", 0)


def flip(w, at):
    out = w.copy()
    out[at, 0] ^= np.uint64(1)
    return out


def test_the_circuit_refuses_what_it_must(el):
    wit, _ = el.witnesses([el.indices[2]], votes=[1])
    w = wit[0]
    assert not el.both_refuse(w)
    two_hot = w.copy(); two_hot[el.block("M") + 3, 0] = 1
    none_hot = w.copy(); none_hot[el.block("M"):el.block("M") + el.n] = 0
    sn_bit = flip(w, el.block("SN_BITS") + 5)
    sn_bit[el.block("SN_PACKED")] = np.array(jm.words(vm.from_words(w[el.block("SN_PACKED")]) ^ 32), np.uint64)
    cases = {"sn_packed": flip(w, el.block("SN_PACKED")), "sn_packed_high": flip(w, el.block("SN_PACKED") + 1), "rt_packed": flip(w, el.block("RT_PACKED")),
             "two_hot": two_hot, "none_hot": none_hot, "address": flip(w, el.block("ADDRESS_BITS") + el.depth - 1), "sk": flip(w, el.block("SK_BITS") + 200),
             "copath": flip(w, el.block("COPATH_BITS") + 255 + 17), "sn_bit": sn_bit}
    for name, bad in cases.items():
        assert el.both_refuse(bad), name


def test_a_digest_has_one_bit_pattern(el, table):
    """voter 1's sn digest u is below 2^255 - r: SN_BITS = bits(u + r) with the consistent packing is the alias that only the strict
    comparison turns away"""
    u = vm.serial_number(table, el.eid, el.sks[1])
    assert u < (1 << 255) - jm.R
    wit, status = el.witnesses([1], votes=[0])
    w = wit[0]
    first = el.block("SN_BITS")
    assert not status.any() and vm.witness_ints(w[first:first + 255]) == jm.bits_of(u, 255)
    bits = jm.bits_of(u + jm.R, 255)
    alias = w.copy()
    alias[first:first + 255] = 0
    alias[first:first + 255, 0] = np.array(bits, np.uint64)
    lo, hi = vm.pack(bits)
    alias[el.block("SN_PACKED")] = np.array(jm.words(lo), np.uint64)
    alias[el.block("SN_PACKED") + 1] = np.array(jm.words(hi), np.uint64)
    assert (lo + (hi << 254)) % jm.R == u                           # the packing rows hold: the same field element
    assert el.both_refuse(alias)


def test_statuses_and_their_neighbours(el3):
    e = el3
    rng = random.Random(5)
    stranger = rng.getrandbits(255)
    good = [(e.sks[0], 0, 0), (e.sks[7], 7, 3), (e.sks[2], 2, 1)]
    bad = [(stranger, 3, 0, 1), (e.sks[4], 4, e.n, 2), (e.sks[4], 8, 0, 2), (e.sks[4] | (1 << 255), 4, 0, 2), (e.sks[5], 4, 1, 1)]
    mixed = [good[0], bad[0][:3], bad[1][:3], good[1], bad[2][:3], bad[3][:3], bad[4][:3], good[2]]
    def run(members):
        return e.circ.witness_batch(e.reg, eid_words(e.eid), np.array([jm.words(m[0], 4) for m in members], np.uint64), [m[1] for m in members], [m[2] for m in members])
    wit, status = run(mixed)
    assert status.tolist() == [0, 1, 2, 0, 2, 2, 1, 0]
    for k in (1, 2, 4, 5, 6):
        assert not wit[k].any()
    alone, s2 = run(good)
    assert not s2.any() and np.array_equal(wit[[0, 3, 7]], alone)
    only_bad, s3 = run([b[:3] for b in bad])
    assert s3.tolist() == [b[3] for b in bad] and not only_bad.any()
    none, s4 = run([bad[1][:3], bad[2][:3]])                        # no member reaches the GPU
    assert s4.tolist() == [2, 2] and not none.any()


def test_argument_errors(ctx, ped, el3, gens):
    lib = ctx.lib
    h = C.c_void_p(None)
    create = lib.vsp_vote_circuit_create
    assert create(None, ped.h, 4, 8, 3, 1, C.byref(h)) == ERR_ARG
    assert create(ctx.h, None, 4, 8, 3, 1, C.byref(h)) == ERR_ARG and create(ctx.h, ped.h, 4, 8, 3, 1, None) == ERR_ARG
    assert create(ctx.h, ped.h, 0, 8, 3, 1, C.byref(h)) == ERR_ARG and create(ctx.h, ped.h, 4, 0, 3, 1, C.byref(h)) == ERR_ARG
    assert create(ctx.h, ped.h, 4, 189 * G - 255 + 1, 3, 1, C.byref(h)) == ERR_ARG and not h.value
    assert create(ctx.h, ped.h, 4, 8, 25, 1, C.byref(h)) == ERR_UNSUPPORTED and not h.value
    two = v.Pedersen(ctx, np.array([jm.point_words(g) for g in gens[:2]], np.uint64))
    assert create(ctx.h, two.h, 4, 8, 3, 1, C.byref(h)) == ERR_ARG and not h.value
    two.free()
    edge = v.VoteCircuit(ctx, ped, 1, 189 * G - 255, 0)              # the longest eid, a tree of one leaf: accepted
    assert edge.blocks["ADDRESS_BITS"][1] == 0 and edge.blocks["EID_PACKED"][1] == 2
    edge.free()
    c = el3.circ
    first, count = C.c_size_t(0), C.c_size_t(0)
    assert lib.vsp_vote_circuit_wires(c.h, 10, C.byref(first), C.byref(count)) == ERR_ARG and lib.vsp_vote_circuit_wires(None, 0, C.byref(first), C.byref(count)) == ERR_ARG
    assert lib.vsp_vote_circuit_sizes(None, None, None, None, None) == ERR_ARG and lib.vsp_vote_circuit_r1cs(None) is None
    assert lib.vsp_vote_circuit_csr(c.h, 3, None, None, None) == ERR_ARG
    sk = key_array([el3.sks[0]]); idx = np.zeros(1, np.uint64); vote = np.zeros(1, np.uint32)
    wit = np.zeros((1, c.num_vars, 4), np.uint64); status = np.zeros(1, np.uint8)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    args = [ctx.h, c.h, el3.reg.h, p(eid_words(el3.eid)), p(sk), p(idx), p(vote), 0, p(wit), p(status)]
    assert lib.vsp_vote_witness_batch(*args) == 0                   # a count of zero with valid pointers
    for i in range(10):
        if i == 7:
            continue
        broken = list(args); broken[i] = None
        assert lib.vsp_vote_witness_batch(*broken) == ERR_ARG, i
    other = v.Registry.build(ctx, ped, el3.pks[:2], 1)
    args[2] = other.h; args[7] = 1
    assert lib.vsp_vote_witness_batch(*args) == ERR_ARG and b"depth" in lib.vsp_last_error(ctx.h)
    other.free()
    with pytest.raises(ValueError):
        c.witness_host(eid_words(el3.eid), jm.words(el3.sks[0]), 8, 0, np.zeros((3, 4), np.uint64))


def test_end_to_end_cast_verify_and_the_ballot_box(ctx, ped, table):
    """depth 2, n 3: a Groth16 key over the circuit, a SAVER key, vsp_vote_cast_batch for three voters of whom one casts twice; the
    verifier accepts all four, a ballot box with the roles FIXED | SERIAL, SERIAL | FIXED, FIXED takes three and names the replay; a ballot
    cast against another registry is turned away for its rt; with prove_check_witness a tampered member is refused"""
    n = 3
    e = Election(ctx, ped, table, 2, 8, n, 1, 901)
    circ, cs = e.circ, e.circ.cs
    kp = v.Keypair(ctx, cs, rand_fr_array(5, 31))
    parts = {k: kp.part(k) for k in ("gamma_ABC_g1", "delta_g1", "gamma_g1", "alpha_g1", "beta_g2", "gamma_g2", "delta_g2")}
    gabc = np.ascontiguousarray(parts["gamma_ABC_g1"])
    pk_w, _, _ = v.saver_generate_keypair(ctx, rand_fr_array(3 * n + 2, 32), gabc, parts["delta_g1"][0], parts["gamma_g1"][0], n)
    spk = v.SaverPublicKey(ctx, pk_w, gabc[:n + 1], n)
    ver = v.SaverVerifier(ctx, pk_w, parts["alpha_g1"][0], parts["beta_g2"][0], parts["gamma_g2"][0], parts["delta_g2"][0], gabc, n)
    voters, votes = [0, 3, 2, 3], [1, 0, 2, 2]
    sks = [e.sks[x] for x in voters]
    rnd = rand_fr_array(12, 33).reshape(3, 4, 4)
    ct, (A, B, Cc), proofs, blobs, status = circ.cast_batch(e.reg, spk, kp.pk, eid_words(e.eid), key_array(sks), voters, votes, rnd[0], rnd[1], rnd[2])
    assert not status.any()
    # what a voter sends beside the ballot, from the library's own hash and registry
    eid_packed = np.array([jm.words(sum(b << i for i, b in enumerate(e.eid)))], np.uint64)
    sn = v.digest_scalars(v.pedersen_hash_batch(ctx, ped, sn_messages(e.eid, sks), e.nbits + 255))
    rt = e.reg.rt_scalars()
    rest = np.stack([np.concatenate([eid_packed, sn[k], rt]) for k in range(4)])
    verdict, reason = v.saver_verify_batch(ctx, ver, ct, rest, A, B, Cc)
    assert verdict.tolist() == [1, 1, 1, 1] and not reason.any()
    expected = np.concatenate([eid_packed, np.zeros((2, 4), np.uint64), rt])
    box = v.BallotBox(ctx, ver, expected, [v.api.FIXED, v.api.SERIAL, v.api.SERIAL, v.api.FIXED, v.api.FIXED])
    verdict, reason, wire, accepted, holder = box.receive_blobs(blobs, proofs, [v.fr_vector_to_blob(r) for r in rest])
    assert verdict.tolist() == [1, 1, 1, 0] and reason.tolist() == [0, 0, 0, 16] and accepted == 3 and holder[3] == 1 and not wire.any()
    # the same voter in another registry: a valid ballot for a tree this box does not serve
    reg2 = v.Registry.build(ctx, ped, e.pks[::-1].copy(), 2, hash_leaves=True)
    ct2, (A2, B2, C2), proofs2, blobs2, status2 = circ.cast_batch(reg2, spk, kp.pk, eid_words(e.eid), key_array([e.sks[1]]), [2], [0], rnd[0][:1], rnd[1][:1], rnd[2][:1])
    sn2 = v.digest_scalars(v.pedersen_hash_batch(ctx, ped, sn_messages(e.eid, [e.sks[1]]), e.nbits + 255))
    rest2 = np.concatenate([eid_packed, sn2[0], reg2.rt_scalars()])[None]
    assert not status2.any() and v.saver_verify_batch(ctx, ver, ct2, rest2, A2, B2, C2)[0].tolist() == [1]
    verdict, reason, _, accepted, _ = box.receive_blobs(blobs2, proofs2, [v.fr_vector_to_blob(rest2[0])])
    assert verdict.tolist() == [0] and reason.tolist() == [8] and accepted == 0
    # an unregistered voter beside a registered one: all-zero outputs, the neighbour as alone
    ct3, (A3, _, _), proofs3, _, status3 = circ.cast_batch(e.reg, spk, kp.pk, eid_words(e.eid), key_array([e.sks[0] ^ 1, sks[1]]), [0, 3], [0, 0], rnd[0][:2], rnd[1][:2], rnd[2][:2])
    assert status3.tolist() == [1, 0] and not ct3[0].any() and not A3[0].any() and proofs3[0] == bytes(192)
    assert np.array_equal(ct3[1], ct[1]) and proofs3[1] == proofs[1]
    # the prover's own gate on a tampered member
    wit, _ = circ.witness_batch(e.reg, eid_words(e.eid), key_array(sks[:2]), voters[:2], votes[:2])
    wit[1, e.block("SK_BITS") + 9, 0] ^= np.uint64(1)
    msgs = np.zeros((2, n, 4), np.uint64); msgs[0, votes[0], 0] = 1; msgs[1, votes[1], 0] = 1
    ctx.set_option("prove_check_witness", 1)
    try:
        with pytest.raises(v.Unsatisfied) as info:
            v.saver_encrypt_batch(ctx, spk, cs, kp.pk, msgs, wit, rnd[0][:2], rnd[1][:2], rnd[2][:2])
    finally:
        ctx.set_option("prove_check_witness", 0)
    assert info.value.status.tolist() == [0, 2]
    assert np.array_equal(info.value.results[0][0], ct[0]) and not info.value.results[0][1].any()
    box.free(); reg2.free(); ver.free(); spk.free(); kp.free(); e.free()
