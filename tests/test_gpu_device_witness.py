"""GPU tests of the device witness source (include/vsp.h "WITNESSES IN DEVICE MEMORY"): the batch prover, the witness
check and the ballot batch over rows of a device buffer against their host forms, byte for byte; the voting circuit's witnesses left on
the device against vsp_vote_witness_batch, word for word; vsp_vote_cast_batch under option vote_cast_device 1 and 0; the cast in two
halves.  Two elections: depth 2, eid_bits 8, n 3 with hashed leaves, and depth 3, eid_bits 8, n 4 with plain leaves.  Device buffers
are torch tensors handed over by data_ptr()."""
import ctypes as C
import random

import numpy as np
import pytest
import torch

import jubjub_model as jm
import vote_circuit_model as vm
import vote_saver_protocol_amd as v
from conftest import rand_fr_array

pytestmark = pytest.mark.gpu

G = 3
OK, ERR_ARG = 0, -1
R_WORDS = np.array(jm.words(jm.R), np.uint64)
SHAPES = {"depth2_hashed": (2, 8, 3, 1), "depth3_plain": (3, 8, 4, 0)}


def key_array(keys):
    return np.array([jm.words(k, 4) for k in keys], np.uint64).reshape(-1, 4)


def eid_words(bits):
    return np.array(jm.message_words(bits), np.uint64)


def sn_messages(eid, sks):
    return np.array([jm.message_words(list(eid) + jm.bits_of(sk, 255)) for sk in sks], np.uint64)


def device_rows(rows):
    """[rows, stride, 4] uint64 -> a torch tensor on the GPU with the same bytes, complete before it is used"""
    t = torch.from_numpy(np.ascontiguousarray(rows).view(np.int64)).cuda()
    torch.cuda.synchronize()
    return t


class Election:
    """a circuit, every leaf of the tree registered, an eid (as tests/test_gpu_vote_circuit.py builds one), and the keys of its ballots:
    a Groth16 key over the circuit, a SAVER key, a verifier"""

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
        self.cs = self.circ.cs
        self.nv = self.circ.num_vars
        self.kp = v.Keypair(ctx, self.cs, rand_fr_array(5, 31 + seed))
        parts = {k: self.kp.part(k) for k in ("gamma_ABC_g1", "delta_g1", "gamma_g1", "alpha_g1", "beta_g2", "gamma_g2", "delta_g2")}
        gabc = np.ascontiguousarray(parts["gamma_ABC_g1"])
        pk_w, _, _ = v.saver_generate_keypair(ctx, rand_fr_array(3 * n + 2, 32 + seed), gabc, parts["delta_g1"][0], parts["gamma_g1"][0], n)
        self.spk = v.SaverPublicKey(ctx, pk_w, gabc[:n + 1], n)
        self.ver = v.SaverVerifier(ctx, pk_w, parts["alpha_g1"][0], parts["beta_g2"][0], parts["gamma_g2"][0], parts["delta_g2"][0], gabc, n)

    def witnesses(self, indices, votes=None, sks=None):
        votes = [i % self.n for i in range(len(indices))] if votes is None else votes
        sks = [self.sks[x] for x in indices] if sks is None else sks
        return self.circ.witness_batch(self.reg, eid_words(self.eid), key_array(sks), indices, votes)

    def members(self, statuses):
        """(sks, indices, votes) of members that end with the given statuses: 1 = sk with a flipped bit, 2 = vote = n"""
        sks, idx, votes = [], [], []
        for k, st in enumerate(statuses):
            x = (k + 1) % (1 << self.depth)
            sks.append(self.sks[x] ^ (1 << 7) if st == 1 else self.sks[x]); idx.append(x); votes.append(self.n if st == 2 else k % self.n)
        return key_array(sks), idx, votes

    def cast(self, statuses, seed=40):
        sks, idx, votes = self.members(statuses)
        rnd = rand_fr_array(3 * len(statuses), seed).reshape(3, len(statuses), 4)
        return (self.reg, self.spk, self.kp.pk, eid_words(self.eid), sks, idx, votes, rnd[0], rnd[1], rnd[2])

    def block(self, name):
        return self.circ.blocks[name][0]

    def free(self):
        self.ver.free(); self.spk.free(); self.kp.free(); self.circ.free(); self.reg.free()


@pytest.fixture(scope="module")
def ped(ctx):
    h = v.Pedersen(ctx, np.array([jm.point_words(g) for g in jm.generators(G)], np.uint64))
    yield h
    h.free()


@pytest.fixture(scope="module")
def table():
    return jm.Table(jm.generators(G))


@pytest.fixture(scope="module", params=list(SHAPES), ids=list(SHAPES))
def el(request, ctx, ped, table):
    e = Election(ctx, ped, table, *SHAPES[request.param], seed=610 + len(request.param))
    yield e
    e.free()


@pytest.fixture(scope="module")
def el2(ctx, ped, table):
    e = Election(ctx, ped, table, *SHAPES["depth2_hashed"], seed=633)
    yield e
    e.free()


def same_ballots(got, want):
    """every output of two ballot batches: ct, (A, B, C), proofs, ct blobs (and the statuses of a cast)"""
    assert np.array_equal(got[0], want[0])
    for a, b in zip(got[1], want[1]):
        assert np.array_equal(a, b)
    assert got[2] == want[2] and got[3] == want[3]
    if len(want) > 4:
        assert got[4].tolist() == want[4].tolist()


def padded(wit, rows, stride, seed):
    """the witnesses as the first values of rows of a wider, longer buffer whose other words are noise"""
    buf = rand_fr_array(rows * stride, seed).reshape(rows, stride, 4)
    buf[:wit.shape[0], :wit.shape[1]] = wit
    return buf


def test_batch_prover_over_device_rows_equals_the_host_form(ctx, el2):
    e = el2
    wit, status = e.witnesses([0, 3, 2])
    assert not status.any()
    stride = e.nv + 3
    buf = padded(wit, 4, stride, 11)                               # row 3 is noise: no member names it
    d = device_rows(buf)
    rnd = rand_fr_array(6, 12).reshape(2, 3, 4)
    members = [2, 0, 2]
    want = v.groth16_prove_batch(ctx, e.cs, e.kp.pk, wit[members], rnd[0], rnd[1])
    got = v.groth16_prove_batch_device(ctx, e.cs, e.kp.pk, d.data_ptr(), stride, 4, rnd[0], rnd[1], members=members)
    for a, b in zip(got[:3], want[:3]):
        assert np.array_equal(a, b)
    assert got[3] == want[3]
    one = v.groth16_prove_batch_device(ctx, e.cs, e.kp.pk, d.data_ptr(), stride, 4, rnd[0][:1], rnd[1][:1], count=1)
    ref = v.groth16_prove_batch(ctx, e.cs, e.kp.pk, wit[:1], rnd[0][:1], rnd[1][:1])
    assert one[3] == ref[3] and np.array_equal(one[0], ref[0]) and np.array_equal(one[1], ref[1]) and np.array_equal(one[2], ref[2])
    assert ctx.stat("prove_witness_h2d_bytes") > 0


def test_witness_check_over_70_device_rows_crosses_the_piece_boundary(ctx, el2):
    e = el2
    idx = [k % (1 << e.depth) for k in range(70)]
    wit, status = e.witnesses(idx)
    assert not status.any()
    sk_bit, zero_wire = e.block("SK_BITS") + 9, e.block("M") + 0
    def tamper(k):
        wit[k, sk_bit, 0] ^= np.uint64(1)
    def value_r(k):
        assert not wit[k, zero_wire + (k + 1) % e.n].any()        # a message slot that holds 0 (the vote is k % n)
        wit[k, zero_wire + (k + 1) % e.n] = R_WORDS
    tamper(5); value_r(9)
    for k in (63, 64):
        tamper(k); value_r(k)
    want = e.cs.check(ctx, wit)
    assert want[0][5] == 2 and want[0][9] == 1 and want[0][63] & want[0][64] & 1 and not want[0][0]
    stride = e.nv + 1
    d = device_rows(padded(wit, 70, stride, 13))
    got = e.cs.check_device(ctx, d.data_ptr(), stride, 70, count=70)
    for a, b in zip(got, want):
        assert np.array_equal(a, b)
    # a map in another order, with a repeat, over the same boundary
    members = list(range(69, -1, -1)) + [64]
    got = e.cs.check_device(ctx, d.data_ptr(), stride, 70, members=members)
    for a, b in zip(got, want):
        assert np.array_equal(a, b[members])


def test_saver_batch_over_device_rows_equals_the_host_form(ctx, el2):
    e = el2
    wit, _ = e.witnesses([0, 3, 2])
    stride = e.nv + 2
    d = device_rows(padded(wit, 5, stride, 14))
    members = [1, 2, 0]
    rnd = rand_fr_array(9, 15).reshape(3, 3, 4)
    host_wit = np.ascontiguousarray(wit[members])
    msgs = np.ascontiguousarray(host_wit[:, :e.n])
    try:
        for gpu in (1, 0):
            ctx.set_option("saver_encrypt_gpu", gpu)
            want = v.saver_encrypt_batch(ctx, e.spk, e.cs, e.kp.pk, msgs, host_wit, rnd[0], rnd[1], rnd[2])
            got = v.saver_encrypt_batch_device(ctx, e.spk, e.cs, e.kp.pk, d.data_ptr(), stride, 5, rnd[0], rnd[1], rnd[2], members=members)
            same_ballots(got, want)
    finally:
        ctx.set_option("saver_encrypt_gpu", 1)
    # the prover's own gate: one tampered member, the same refusal, verdicts and zeroed member
    bad = wit.copy()
    bad[2, e.block("SK_BITS") + 9, 0] ^= np.uint64(1)
    d_bad = device_rows(padded(bad, 5, stride, 16))
    host_bad = np.ascontiguousarray(bad[members])
    ctx.set_option("prove_check_witness", 1)
    try:
        with pytest.raises(v.Unsatisfied) as want:
            v.saver_encrypt_batch(ctx, e.spk, e.cs, e.kp.pk, msgs, host_bad, rnd[0], rnd[1], rnd[2])
        with pytest.raises(v.Unsatisfied) as got:
            v.saver_encrypt_batch_device(ctx, e.spk, e.cs, e.kp.pk, d_bad.data_ptr(), stride, 5, rnd[0], rnd[1], rnd[2], members=members)
    finally:
        ctx.set_option("prove_check_witness", 0)
    assert got.value.status.tolist() == want.value.status.tolist() == [0, 2, 0]
    assert got.value.first_bad_row.tolist() == want.value.first_bad_row.tolist()
    same_ballots(got.value.results, want.value.results)
    assert not got.value.results[0][1].any() and got.value.results[2][1] == bytes(192) and got.value.results[0][0].any()


def test_a_value_not_below_r_is_refused_by_the_finish_for_the_whole_batch(ctx, el2):
    """the device form's launch never sees the message: the multi-exponentiations' census finds the value and the finish refuses the
    batch, as the batch prover does for a host witness, and no ciphertext leaves; the context proves normally afterwards"""
    e = el2
    wit, _ = e.witnesses([0, 3])
    good = device_rows(wit)
    big = wit.copy()
    big[1, e.block("M") + 2] = R_WORDS                              # member 1 votes 1: slot 2 holds 0, and r is 0 mod r
    assert not wit[1, e.block("M") + 2].any()
    d = device_rows(big)
    rnd = rand_fr_array(6, 19).reshape(3, 2, 4)
    lib = ctx.lib
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    with pytest.raises(v.VspError) as host:
        v.groth16_prove_batch(ctx, e.cs, e.kp.pk, big, rnd[1], rnd[2])
    assert not isinstance(host.value, v.Unsatisfied)
    ct = np.ones((2, e.n + 2, 12), np.uint64); blobs = np.ones((2, lib.vsp_g1_vector_blob_size(e.n + 2)), np.uint8)
    assert lib.vsp_saver_encrypt_batch_launch_device(ctx.h, e.spk.h, e.cs.h, e.kp.pk.h, C.c_void_p(d.data_ptr()), e.nv, 2, None, 2, p(rnd[0]), p(rnd[1]), p(rnd[2])) == OK
    assert lib.vsp_saver_encrypt_batch_finish(ctx.h, p(ct), None, None, None, None, p(blobs)) == ERR_ARG
    assert ctx.last_error() in str(host.value) and not ct.any() and not blobs.any()
    want = v.saver_encrypt_batch(ctx, e.spk, e.cs, e.kp.pk, np.ascontiguousarray(wit[:, :e.n]), wit, rnd[0], rnd[1], rnd[2])
    same_ballots(v.saver_encrypt_batch_device(ctx, e.spk, e.cs, e.kp.pk, good.data_ptr(), e.nv, 2, rnd[0], rnd[1], rnd[2], count=2), want)


def test_device_witnesses_equal_the_host_call_and_release_zeroes_them(ctx, el):
    e = el
    sks, idx, votes = e.members([0, 1, 2, 0])
    want, want_status = e.circ.witness_batch(e.reg, eid_words(e.eid), sks, idx, votes)
    d2h_before = ctx.stat("vote_witness_d2h_bytes")
    dptr, stride, status = e.circ.witness_batch_device(e.reg, eid_words(e.eid), sks, idx, votes)
    assert ctx.stat("vote_witness_d2h_bytes") == d2h_before
    assert status.tolist() == want_status.tolist() == [0, 1, 2, 0] and stride == e.nv and dptr
    got = np.zeros((4, stride, 4), np.uint64)
    ctx.d2h(got, dptr)
    assert np.array_equal(got, want) and got[0].any() and not got[1].any() and not got[2].any()
    # the rows are a source for the checker where they lie
    verdict, _, _ = e.cs.check_device(ctx, dptr, stride, 4, members=[3, 0])
    assert not verdict.any()
    e.circ.witness_release()
    ctx.d2h(got, dptr)
    assert not got.any()
    # a second device call releases the first one's rows: one member now, the rows beyond it read zero
    dptr2, _, status2 = e.circ.witness_batch_device(e.reg, eid_words(e.eid), sks[3:], idx[3:], votes[3:])
    assert dptr2 == dptr and status2.tolist() == [0]
    ctx.d2h(got, dptr)
    assert np.array_equal(got[0], want[3]) and not got[1:].any()
    # and so does the host call
    e.circ.witness_batch(e.reg, eid_words(e.eid), sks[:1], idx[:1], votes[:1])
    ctx.d2h(got, dptr)
    assert not got.any()


@pytest.mark.parametrize("statuses", [[0, 0, 0, 0], [1, 0], [0, 2, 1], [2, 1]], ids=lambda s: "status_" + "".join(map(str, s)))
def test_cast_is_the_same_under_both_options(ctx, el, statuses):
    e = el
    args = e.cast(statuses)
    count, live = len(statuses), statuses.count(0)
    moved = {}
    out = {}
    try:
        for opt in (1, 0):
            ctx.set_option("vote_cast_device", opt)
            before = (ctx.stat("vote_witness_d2h_bytes"), ctx.stat("prove_witness_h2d_bytes"))
            out[opt] = e.circ.cast_batch(*args)
            moved[opt] = (ctx.stat("vote_witness_d2h_bytes") - before[0], ctx.stat("prove_witness_h2d_bytes") - before[1])
    finally:
        ctx.set_option("vote_cast_device", 1)
    assert out[1][4].tolist() == statuses
    same_ballots(out[1], out[0])
    for k, st in enumerate(statuses):
        assert out[1][0][k].any() == (st == 0) and (out[1][2][k] != bytes(192)) == (st == 0)
    assert moved[1] == (0, 0)
    assert moved[0] == (32 * e.nv * count, 32 * e.nv * live)


def test_cast_is_the_same_under_both_options_with_the_provers_gate(ctx, el2):
    e = el2
    args = e.cast([0, 2, 1], seed=41)
    out = {}
    ctx.set_option("prove_check_witness", 1)
    try:
        for opt in (1, 0):
            ctx.set_option("vote_cast_device", opt)
            out[opt] = e.circ.cast_batch(*args)
    finally:
        ctx.set_option("vote_cast_device", 1); ctx.set_option("prove_check_witness", 0)
    same_ballots(out[1], out[0])
    assert out[1][4].tolist() == [0, 2, 1] and out[1][0][0].any()


def test_cast_in_two_halves_and_its_misuse(ctx, el2):
    e = el2
    lib = ctx.lib
    args = e.cast([0, 1, 0], seed=42)
    want = e.circ.cast_batch(*args)
    none = [None] * 6
    assert lib.vsp_cast_batch_finish(ctx.h, *none) == ERR_ARG and b"no batch" in lib.vsp_last_error(ctx.h)
    status = e.circ.cast_batch_launch(*args)
    assert status.tolist() == [0, 1, 0]
    # in flight: a second launch and a prover call are refused, and the batch is still there
    with pytest.raises(v.VspError, match="in flight"):
        e.circ.cast_batch_launch(*args)
    wit, _ = e.witnesses([0])
    rnd = rand_fr_array(2, 43).reshape(2, 1, 4)
    with pytest.raises(v.VspError, match="in flight"):
        v.groth16_prove_batch_launch(ctx, e.cs, e.kp.pk, wit, rnd[0], rnd[1])
    with pytest.raises(v.VspError, match="in flight"):
        e.cs.check(ctx, wit)
    same_ballots(e.circ.cast_batch_finish(), want)
    assert lib.vsp_cast_batch_finish(ctx.h, *none) == ERR_ARG
    # a batch without a live member is in flight too, and finishes into zeros
    dead = e.cast([2, 1], seed=44)
    assert e.circ.cast_batch_launch(*dead).tolist() == [2, 1]
    with pytest.raises(v.VspError, match="in flight"):
        v.groth16_prove_batch_launch(ctx, e.cs, e.kp.pk, wit, rnd[0], rnd[1])
    ct, (A, B, Cc), proofs, blobs, st = e.circ.cast_batch_finish()
    assert not ct.any() and not A.any() and not B.any() and not Cc.any() and proofs == [bytes(192)] * 2 and st.tolist() == [2, 1]
    # the context proves normally afterwards
    ref = v.groth16_prove_batch(ctx, e.cs, e.kp.pk, wit, rnd[0], rnd[1])
    assert ref[3][0] != bytes(192)
    same_ballots(e.circ.cast_batch(*args), want)


def test_two_contexts_alternate_their_casts(ctx, ped, el2):
    """a thread with two contexts and two circuits: the second batch's witnesses are built while the first batch proves"""
    e = el2
    other = v.Context(0)
    try:
        circ2 = v.VoteCircuit(other, ped, e.n, e.nbits, e.depth, hash_leaves=bool(e.hash_leaves))
        a, b = e.cast([0, 0, 1], seed=45), e.cast([0, 2, 0, 0], seed=46)
        want_a, want_b = e.circ.cast_batch(*a), e.circ.cast_batch(*b)
        e.circ.cast_batch_launch(*a)
        circ2.cast_batch_launch(*b)
        same_ballots(e.circ.cast_batch_finish(), want_a)
        same_ballots(circ2.cast_batch_finish(), want_b)
        circ2.free()
    finally:
        other.close()


def test_argument_errors_and_a_device_ballot_verifies(ctx, ped, el2):
    e = el2
    lib = ctx.lib
    wit, _ = e.witnesses([0, 3])
    stride = e.nv + 1
    d = device_rows(padded(wit, 2, stride, 17))
    rnd = rand_fr_array(6, 18).reshape(3, 2, 4)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    members = np.array([1, 0], np.uint32)
    def launch(d_wit=d.data_ptr(), stride=stride, rows=2, members=members, count=2, cs=e.cs.h, pk=e.kp.pk.h, r=rnd[1]):
        rc = lib.vsp_groth16_prove_batch_launch_device(ctx.h, cs, pk, C.c_void_p(d_wit) if d_wit else None, stride, rows, p(members) if members is not None else None, count,
                                                       p(r) if r is not None else None, p(rnd[2]))
        return rc, lib.vsp_last_error(ctx.h)
    assert lib.vsp_groth16_prove_batch_launch_device(None, e.cs.h, e.kp.pk.h, C.c_void_p(d.data_ptr()), stride, 2, None, 2, p(rnd[1]), p(rnd[2])) == ERR_ARG
    for broken in (dict(d_wit=None), dict(cs=None), dict(pk=None), dict(r=None), dict(count=0), dict(count=65)):
        rc, msg = launch(**broken)
        assert rc == ERR_ARG and b"null argument or a batch outside 1..64" in msg, broken
    rc, msg = launch(stride=e.nv - 1)
    assert rc == ERR_ARG and b"stride" in msg and b"below num_vars" in msg
    rc, msg = launch(members=np.array([1, 2], np.uint32))
    assert rc == ERR_ARG and b"members[1] = 2 is not a row" in msg
    rc, msg = launch(members=None, count=3)
    assert rc == ERR_ARG and b"count exceeds the rows" in msg
    rc, msg = launch(d_wit=d.data_ptr() + 8)
    assert rc == ERR_ARG and b"16-byte aligned" in msg
    # the same refusals from the checker and the ballot batch, under their own names
    st = np.zeros(2, np.uint8)
    assert lib.vsp_r1cs_check_batch_device(ctx.h, e.cs.h, C.c_void_p(d.data_ptr()), e.nv - 1, 2, None, 2, p(st), None, None) == ERR_ARG
    assert b"r1cs_check_device" in lib.vsp_last_error(ctx.h)
    assert lib.vsp_r1cs_check_batch_device(ctx.h, e.cs.h, None, stride, 2, None, 2, p(st), None, None) == ERR_ARG
    bad = np.array([0, 7], np.uint32)
    assert lib.vsp_saver_encrypt_batch_launch_device(ctx.h, e.spk.h, e.cs.h, e.kp.pk.h, C.c_void_p(d.data_ptr()), stride, 2, p(bad), 2, p(rnd[0]), p(rnd[1]), p(rnd[2])) == ERR_ARG
    assert b"saver_encrypt_batch_device: members[1] = 7" in lib.vsp_last_error(ctx.h)
    assert lib.vsp_saver_encrypt_batch_launch_device(ctx.h, e.spk.h, e.cs.h, e.kp.pk.h, None, stride, 2, None, 2, p(rnd[0]), p(rnd[1]), p(rnd[2])) == ERR_ARG
    big = rnd[0].copy(); big[1] = R_WORDS
    assert lib.vsp_saver_encrypt_batch_launch_device(ctx.h, e.spk.h, e.cs.h, e.kp.pk.h, C.c_void_p(d.data_ptr()), stride, 2, None, 2, p(big), p(rnd[1]), p(rnd[2])) == ERR_ARG
    assert b"r_enc of member 1" in lib.vsp_last_error(ctx.h)
    # a proof in flight
    rc, _ = launch()
    assert rc == OK
    rc, msg = launch()
    assert rc == ERR_ARG and b"in flight" in msg
    assert lib.vsp_r1cs_check_batch_device(ctx.h, e.cs.h, C.c_void_p(d.data_ptr()), stride, 2, None, 2, p(st), None, None) == ERR_ARG
    proofs = np.zeros((2, 192), np.uint8)
    assert lib.vsp_groth16_prove_batch_finish(ctx.h, None, None, None, p(proofs)) == OK
    want = v.groth16_prove_batch(ctx, e.cs, e.kp.pk, wit[[1, 0]], rnd[1], rnd[2])
    assert [proofs[k].tobytes() for k in range(2)] == want[3]
    # handles of the witness call
    dp, sd = C.c_void_p(None), C.c_size_t(0)
    sks, idx, votes = e.members([0])
    votes = np.array(votes, np.uint32); idx = np.array(idx, np.uint64)
    wargs = [ctx.h, e.circ.h, e.reg.h, p(eid_words(e.eid)), p(sks), p(idx), p(votes), 1, C.byref(dp), C.byref(sd), p(st)]
    for i in (1, 2, 3, 4, 5, 6, 8, 9, 10):
        broken = list(wargs); broken[i] = None
        assert lib.vsp_cast_witness_batch_device(*broken) == ERR_ARG, i
    for count in (0, 65):
        broken = list(wargs); broken[7] = count
        assert lib.vsp_cast_witness_batch_device(*broken) == ERR_ARG and b"1 to 64" in lib.vsp_last_error(ctx.h)
    assert lib.vsp_cast_witness_release(ctx.h, None) == ERR_ARG and lib.vsp_cast_witness_release(None, e.circ.h) == ERR_ARG
    # both paths equally wrong would still agree with each other: a ballot of the device path before the verifier
    ctx.set_option("vote_cast_device", 1)
    voters, votes = [0, 3], [1, 0]
    sks = [e.sks[x] for x in voters]
    ct, (A, B, Cc), _, _, status = e.circ.cast_batch(e.reg, e.spk, e.kp.pk, eid_words(e.eid), key_array(sks), voters, votes, rnd[0], rnd[1], rnd[2])
    assert not status.any()
    eid_packed = np.array([jm.words(sum(b << i for i, b in enumerate(e.eid)))], np.uint64)
    sn = v.digest_scalars(v.pedersen_hash_batch(ctx, ped, sn_messages(e.eid, sks), e.nbits + 255))
    rest = np.stack([np.concatenate([eid_packed, sn[k], e.reg.rt_scalars()]) for k in range(2)])
    verdict, reason = v.saver_verify_batch(ctx, e.ver, ct, rest, A, B, Cc)
    assert verdict.tolist() == [1, 1] and not reason.any()
